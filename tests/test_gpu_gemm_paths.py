"""cg_gemm on the kernels and routes no other op test takes -- the scalar-epilogue bf16 fallback
(gemm_bf16_kernel), the 64x64 fp32 kernel, the scalar split-K reducer, split-K with an epilogue,
the unfused column-sum fallback -- and every forced bf16 tile, all under one forward-error bound
against the fp64 product of the same (bf16-rounded) operands:

    |out - ref| <= 2e-5 S + (bf16 output) 2^-8 |ref| + 1e-30

S is the epilogue evaluated on absolute values: |alpha| (|A| |B|^T), plus |bias|, |resid|, |acc0|
where they take part, times 1 / (1 - p) on kept dropout elements, times 1.13 (max |gelu'|) through
GELU, times |gelu'(aux)| through DGELU.  2e-5 is test_gemm_layouts' constant (a few fp32 ulps of
the accumulated magnitudes for K <= 1024).  Column sums: 2e-5 sum_rows S per column.

Every test needs the MI355X (marker ``gpu``) and calls the C ABI through codonlm_amd.ops.
"""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import tinygpt_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
LAYOUTS = [(1, 1), (1, 0), (0, 0), (0, 1)]
DROP_P, DROP_SEED = 0.25, 12345
# DGELU multiplies the product v by gelu'(aux) = Phi(a) + a phi(a) evaluated in fp32.  Phi comes
# from 0.5 (1 + erf(a / sqrt 2)), whose sum cancels for negative a, so gelu' carries an ABSOLUTE
# error of a few ulps of 1 however small it is; S0 |gelu'| alone (a purely relative bound) cannot
# cover it where |gelu'| is below ~1e-3 (a <= -4, or a near the zero of gelu' at -0.75).  The
# bound therefore adds DGELU_EVAL |v| with DGELU_EVAL = 4 ulp(1) = 4.8e-7: one ulp each for erf,
# the 1 + erf sum, the Gaussian factor and the final sum.  Measured on the MI355X without the
# term: err / bound up to 9.0 on the bf16 scalar-epilogue kernel (worst element at gelu' =
# -3.5e-7) and up to 1.2e3 on the fp32 64x64 kernel (at gelu' = -1.2e-8), while the vector
# epilogues' polynomial Phi stays below 1; with it: 0.05 at most on the fp32 kernel.
DGELU_EVAL = 4 * 2.0 ** -23


def _mods():
    from codonlm_amd import _lib, ops
    return ops, _lib


def _gelu(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def _dgelu(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


@functools.lru_cache(maxsize=None)
def _problem(dtype, M, N, K):
    """Operands (already rounded to `dtype`), epilogue inputs, and the fp64 product and its
    absolute-value companion: computed once per shape and shared (read-only)."""
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K, generator=g).to(dtype).float()
    B = (torch.randn(N, K, generator=g) * 0.3).to(dtype).float()
    return dict(A=A, B=B, bias=torch.randn(N, generator=g), resid=torch.randn(M, N, generator=g),
                acc0=torch.randn(M, N, generator=g), base=A.double() @ B.double().t(),
                S0=A.double().abs() @ B.double().abs().t(),
                keep=torch.from_numpy(O.dropout_keep(DROP_SEED, np.arange(M)[:, None], np.arange(N)[None, :], DROP_P)))


def _operands(pb, dtype, ak, bk, a_offset=False):
    a = (pb["A"] if ak else pb["A"].t().contiguous()).to(DEV, dtype)
    b = (pb["B"] if bk else pb["B"].t().contiguous()).to(DEV, dtype)
    if a_offset:   # the same operand one element past an aligned base
        buf = torch.empty(a.numel() + 4, dtype=dtype, device=DEV)
        buf[1:1 + a.numel()] = a.view(-1)
        a = buf[1:1 + a.numel()].view(a.shape)
    return a, b


def _ratio(out, ref, S, bf16_out):
    bound = 2e-5 * S + (2.0 ** -8 * ref.abs() if bf16_out else 0.0) + 1e-30
    return ((out.detach().cpu().double() - ref).abs() / bound).max().item()


class _Runner:
    """One (shape, layout, route) under test: runs an epilogue, checks it against the bound, checks
    that nothing outside the [M][N] view of the output buffer was written."""

    def __init__(self, dtype, M, N, K, ak=1, bk=1, *, ldc_pad=0, bias_offset=False, a_offset=False, tag="", **gemm_kw):
        self.ops, self.L = _mods()
        self.dtype, self.M, self.N, self.K = dtype, M, N, K
        self.pb = _problem(dtype, M, N, K)
        self.a, self.b = _operands(self.pb, dtype, ak, bk, a_offset)
        self.kw = dict(a_kcontig=bool(ak), b_kcontig=bool(bk), M=M, N=N, K=K, **gemm_kw)
        self.ldc_pad = ldc_pad
        bias_buf = torch.zeros(N + 8, device=DEV)
        off = 1 if bias_offset else 0
        bias_buf[off:off + N] = self.pb["bias"].to(DEV)
        self.bias = bias_buf[off:off + N]
        assert self.bias.data_ptr() % 16 == (4 if bias_offset else 0)
        self.resid = self.pb["resid"].to(DEV)
        self.tag = f"{tag} {str(dtype)[6:]} {M}x{N}x{K} ak{ak} bk{bk}"
        self.worst = 0.0
        # the narrow output type of this operand type (fp32 operands keep fp32 buffers)
        self.narrow = BF16 if dtype == BF16 else F32

    def _out(self, dt, init=None):
        buf = torch.full((self.M, self.N + self.ldc_pad), float("nan"), dtype=dt, device=DEV)
        view = buf[:, :self.N]
        if init is not None:
            view.copy_(init.to(DEV))
        return buf, view

    def _done(self, name, r, buf):
        torch.cuda.synchronize()
        print(f"gemm {self.tag} {name}: err/bound {r:.4f}")
        self.worst = max(self.worst, r)
        assert r <= 1.0, (self.tag, name, r)
        if self.ldc_pad:
            assert torch.isnan(buf[:, self.N:]).all(), (self.tag, name)

    def run(self, name, **extra):
        L, pb = self.L, self.pb
        base, S0 = pb["base"], pb["S0"]
        bias, resid = pb["bias"].double(), pb["resid"].double()
        kw = dict(self.kw, **extra)
        gemm = self.ops.gemm
        if name == "none":
            buf, out = self._out(F32)
            gemm(self.a, self.b, out=out, **kw)
            self._done(name, _ratio(out, base, S0, False), buf)
        elif name == "none_narrow":
            buf, out = self._out(self.narrow)
            gemm(self.a, self.b, out=out, **kw)
            self._done(name, _ratio(out, base, S0, self.narrow == BF16), buf)
        elif name == "bias":
            buf, out = self._out(self.narrow)
            gemm(self.a, self.b, out=out, bias=self.bias, epilogue=L.EPI_BIAS, **kw)
            self._done(name, _ratio(out, base + bias, S0 + bias.abs(), self.narrow == BF16), buf)
        elif name == "gelu_pair":      # BIAS|GELU + aux_out, then DGELU from that aux
            nb = self.narrow == BF16
            buf, out = self._out(self.narrow)
            aux = torch.full((self.M, self.N), float("nan"), dtype=self.narrow, device=DEV)
            gemm(self.a, self.b, out=out, bias=self.bias, epilogue=L.EPI_BIAS | L.EPI_GELU, aux_out=aux, **kw)
            pre, Sp = base + bias, S0 + bias.abs()
            self._done("bias_gelu aux_out", _ratio(aux, pre, Sp, nb), buf)
            self._done("bias_gelu", _ratio(out, _gelu(pre), 1.13 * Sp, nb), buf)
            buf, out = self._out(self.narrow)
            gemm(self.a, self.b, out=out, epilogue=L.EPI_DGELU, aux=aux, **kw)
            f = _dgelu(aux.cpu().double())
            rel = (out.cpu().double() - base * f).abs() / (2e-5 * S0 * f.abs() + (2.0 ** -8 * (base * f).abs() if nb else 0.0)
                                                          + 1e-30)
            at = rel.argmax()
            print(f"gemm {self.tag} dgelu under 2e-5 S0 |gelu'| alone: err/bound {rel.max().item():.2f} "
                  f"at gelu' = {f.view(-1)[at].item():.2e}")
            self._done("dgelu", _ratio(out, base * f, S0 * f.abs() + DGELU_EVAL / 2e-5 * base.abs(), nb), buf)
        elif name == "bias_drop_resid":
            buf, out = self._out(F32)
            gemm(self.a, self.b, out=out, bias=self.bias, resid=self.resid, drop_seed=DROP_SEED, drop_p=DROP_P,
                 epilogue=L.EPI_BIAS | L.EPI_DROPOUT | L.EPI_RESID, **kw)
            k = pb["keep"].double() / (1 - DROP_P)
            self._done(name, _ratio(out, resid + k * (base + bias), k * (S0 + bias.abs()) + resid.abs(), False), buf)
        elif name == "bias_resid":
            buf, out = self._out(F32)
            gemm(self.a, self.b, out=out, bias=self.bias, resid=self.resid, epilogue=L.EPI_BIAS | L.EPI_RESID, **kw)
            self._done(name, _ratio(out, base + bias + resid, S0 + bias.abs() + resid.abs(), False), buf)
        elif name == "resid":
            buf, out = self._out(F32)
            gemm(self.a, self.b, out=out, resid=self.resid, epilogue=L.EPI_RESID, **kw)
            self._done(name, _ratio(out, base + resid, S0 + resid.abs(), False), buf)
        elif name == "accum":
            acc0 = pb["acc0"]
            buf, out = self._out(F32, init=acc0)
            gemm(self.a, self.b, out=out, epilogue=L.EPI_ACCUM, alpha=0.5, **kw)
            self._done(name, _ratio(out, acc0.double() + 0.5 * base, 0.5 * S0 + acc0.double().abs(), False), buf)
        elif name == "colsum":
            # fp32 C: the column sums of the product itself
            buf, out = self._out(F32)
            cs = torch.full((self.N,), float("nan"), device=DEV)
            gemm(self.a, self.b, out=out, colsum_out=cs, **kw)
            self._done("colsum C", _ratio(out, base, S0, False), buf)
            self._done("colsum sums", _ratio(cs, base.sum(0), S0.sum(0), False), buf)
            if self.narrow == BF16:
                # bf16 C: the fallback sums the rounded C it reads back, so the reference is the
                # fp64 column sum of the C it wrote
                buf, out = self._out(BF16)
                gemm(self.a, self.b, out=out, colsum_out=cs, **kw)
                self._done("colsum C bf16", _ratio(out, base, S0, True), buf)
                c64 = out.cpu().double()
                self._done("colsum sums bf16", _ratio(cs, c64.sum(0), c64.abs().sum(0), False), buf)
        else:
            raise KeyError(name)


FALLBACK_EPIS = ["none", "bias", "gelu_pair", "bias_drop_resid", "accum", "colsum"]


def _fallback_list(r, split_k):
    for name in FALLBACK_EPIS:
        r.run(name)
    r.run("bias", split_k=split_k)           # split-K with an epilogue on the scalar reducer
    r.run("gelu_pair", split_k=split_k)
    r.run("accum", split_k=split_k)
    return r.worst


# ---------------------------------------------------------------------------------------------
# (a) gemm_bf16_kernel: the bf16 path when vec_ok() is false
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K,ak", [(200, 69, 72, 1), (130, 100, 136, 1), (136, 69, 64, 0)])
def test_bf16_fallback_by_n(M, N, K, ak):
    """N % 8 != 0: every epilogue on the scalar-epilogue kernel, the unfused colsum64_kernel, and
    split_k = 2 (K 72 = 64 + 8, K 136 = 128 + 8: a last slab of one 8-element chunk; K 64 gives one
    slab) through splitk_reduce_kernel.  M 200 / 130 / 136: two row tiles, the second ragged."""
    _fallback_list(_Runner(BF16, M, N, K, ak, 1, tag="fallback N%8"), 2)


def test_bf16_fallback_by_ldc():
    """N = 72 and every pointer aligned, but the output a view with ldc = 75: the columns of the
    output buffer past N stay untouched."""
    _fallback_list(_Runner(BF16, 200, 72, 72, ldc_pad=3, tag="fallback ldc%8"), 2)


def test_bf16_fallback_by_bias_pointer():
    """N = 72, ldc = 72, the bias one float past a 16-B boundary: the epilogues that read it."""
    r = _Runner(BF16, 200, 72, 72, bias_offset=True, tag="fallback bias ptr")
    for name in ("bias", "gelu_pair", "bias_drop_resid"):
        r.run(name)
    r.run("bias", split_k=2)


def test_bf16_n_not_multiple_of_8_needs_k_contiguous_b():
    ops, _ = _mods()
    a = torch.zeros(200, 72, dtype=BF16, device=DEV)
    b = torch.zeros(72, 69, dtype=BF16, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm(a, b, b_kcontig=False, M=200, N=69, K=72)


# ---------------------------------------------------------------------------------------------
# (b) gemm_f32_kernel (64x64)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ak,bk", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(70, 50, 37), (65, 65, 17)])
def test_f32_small_tile(M, N, K, ak, bk):
    """fp32 operands whose extents are no multiples of 4 (K % 4 != 0 with a K-contiguous operand,
    M % 4 / N % 4 != 0 with none) take the 64x64 tile: two tiles in M and N, a k-tail of 5 / 1, every
    epilogue with fp32 buffers, the scalar reducer (split_k = 3: K 37 gives slabs of 16 / 16 / 5,
    K 17 two slabs) and the unfused column sum."""
    _fallback_list(_Runner(F32, M, N, K, ak, bk, tag="f32 64x64"), 3)


def test_f32_small_tile_by_pointer():
    """Extents all multiples of 4, A one float past a 16-B boundary."""
    r = _Runner(F32, 72, 64, 32, a_offset=True, tag="f32 64x64 A ptr")
    assert r.a.data_ptr() % 16 == 4
    _fallback_list(r, 2)


# ---------------------------------------------------------------------------------------------
# (c) every forced bf16 tile at the tight bound
# ---------------------------------------------------------------------------------------------
TILE_EPIS = ["none", "accum", "bias_resid", "bias_drop_resid", "resid", "bias", "gelu_pair"]


@pytest.mark.parametrize("ak,bk", LAYOUTS)
@pytest.mark.parametrize("tile,K", [("VEC", 320), ("VEC", 72), ("VEC", 1000), ("WIDE", 320)])
def test_forced_tile_layouts(tile, K, ak, bk):
    """CG_TILE_VEC (128x128 register-staged; K 72 and 1000 end in an 8-element k-chunk) and
    CG_TILE_WIDE (256x128 LDS-DMA) at (520, 264, K): ragged M and N tiles, all four operand
    layouts, fp32 and bf16 epilogues.  (test_gemm_wide_tile allows 2e-2 sqrt(K) here.)"""
    _, L = _mods()
    r = _Runner(BF16, 520, 264, K, ak, bk, tag=f"tile {tile}", tile=getattr(L, "TILE_" + tile))
    for name in TILE_EPIS:
        r.run(name)


@pytest.mark.parametrize("max_wg", [0, 3])
@pytest.mark.parametrize("tile", ["PERS", "PERS_LW"])
def test_forced_persistent_tiles(tile, max_wg):
    """The eight-wave and loader-wave persistent tiles at (520, 264, 320), one workgroup per tile
    and (max_wg = 3) three workgroups that each walk two tiles.  (test_gemm_persistent_tile_epilogues
    allows 0.12 absolute here.)"""
    _, L = _mods()
    r = _Runner(BF16, 520, 264, 320, tag=f"tile {tile} wg{max_wg}", tile=getattr(L, "TILE_" + tile), max_wg=max_wg)
    for name in TILE_EPIS + ["none_narrow"]:
        r.run(name)


# ---------------------------------------------------------------------------------------------
# (d) split-K with an epilogue on the vector reducer
# ---------------------------------------------------------------------------------------------
def test_splitk_vec_reducer_epilogues():
    """bf16, N % 8 == 0, split_k = 2 at (256, 192, 256): splitk_reduce_vec_kernel applies
    BIAS|GELU (+ aux_out, then DGELU from it), BIAS|RESID and BIAS|DROPOUT|RESID to the summed slabs."""
    r = _Runner(BF16, 256, 192, 256, tag="splitk vec", split_k=2)
    for name in ("gelu_pair", "bias_resid", "bias_drop_resid", "bias", "accum"):
        r.run(name)


# ---------------------------------------------------------------------------------------------
# (e) degenerate calls
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("M,N", [(0, 72), (64, 0), (0, 0)])
def test_empty_products_write_nothing(dtype, M, N):
    ops, L = _mods()
    a = torch.ones(64, 64, dtype=dtype, device=DEV)
    b = torch.ones(72, 64, dtype=dtype, device=DEV)
    out = torch.full((64, 72), 5.0, device=DEV)
    bias = torch.ones(72, device=DEV)
    ops.gemm(a, b, M=M, N=N, K=64, out=out)
    ops.gemm(a, b, M=M, N=N, K=64, out=out, bias=bias, epilogue=L.EPI_BIAS | L.EPI_ACCUM)
    torch.cuda.synchronize()
    assert torch.all(out == 5.0)
