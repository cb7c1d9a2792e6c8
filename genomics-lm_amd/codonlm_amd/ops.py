"""Tensor-level wrappers over the op entry points of libcodonlm_hip.so.

Each wrapper validates shapes, allocates outputs with torch on the tensor's device and
launches on the current HIP stream.  These are the building blocks the engine uses
natively; they are exposed for op-level parity tests and for callers that compose
their own step (e.g. the auxiliary heads).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

_DT = {torch.float32: L.CG_F32, torch.bfloat16: L.CG_BF16}


def _dt(t: torch.Tensor) -> int:
    if t.dtype not in _DT:
        raise ValueError(f"unsupported dtype {t.dtype}")
    return _DT[t.dtype]


def _p(t):
    return None if t is None else t.data_ptr()


class _Result:
    """Base of the result classes: every slot None unless given, in slot order or by keyword."""
    __slots__ = ()

    def __init__(self, *args, **given):
        for k in self.__slots__:
            setattr(self, k, None)
        for k, v in zip(self.__slots__, args):
            setattr(self, k, v)
        for k, v in given.items():  # a name that is no slot is an AttributeError
            setattr(self, k, v)


def _check_want(what, want, allowed):
    unknown = set(want) - set(allowed)
    if unknown:
        raise ValueError(f"{what}: unknown outputs {sorted(unknown)}")


def _alloc_outputs(desc, res, want, dev, table, zero=()):
    """For each (name, shape, dtype) of ``table`` named in ``want``: allocate the tensor (torch.empty;
    torch.zeros for the names in ``zero``), set it on ``res`` and its pointer on ``desc`` (None: the
    entry point takes the pointers as arguments)."""
    for name, shape, dt in table:
        if name in want:
            t = (torch.zeros if name in zero else torch.empty)(shape, dtype=dt, device=dev)
            setattr(res, name, t)
            if desc is not None:
                setattr(desc, name, t.data_ptr())


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def _set_ws(desc, ws):
    desc.workspace, desc.ws_bytes = ws.data_ptr(), _nbytes(ws)


def _alloc_ws(need, dev, kind):
    """A workspace of at least ``need`` bytes: "f64" = fp64 of need // 8 + 1 (8-byte aligned, the
    accumulating ops), "u8" = uint8 of max(need, 16), "u8_256" = uint8 of max(need, 256)."""
    need = int(need)
    if kind == "f64":
        return torch.empty(need // 8 + 1, dtype=torch.float64, device=dev)
    return torch.empty(max(need, {"u8": 16, "u8_256": 256}[kind]), dtype=torch.uint8, device=dev)


def _pick_ws(ws, dev, kind, grow, need, *args):
    """The workspace of a launch.  ``grow`` False: the caller's ``ws`` as given (the library answers
    a short one with CG_EINVAL), a fresh one only without it.  ``grow`` True: the caller's if it
    holds the bytes, else a fresh one.  ``need(*args)`` is the library's sizing entry point, asked
    only when it decides something; ``args`` are Python ints (ctypes converts them, nothing else)."""
    if ws is not None and not grow:
        return ws
    n = int(need(*args))
    return ws if ws is not None and _nbytes(ws) >= n else _alloc_ws(n, dev, kind)


def _row_matrix(t, what, dtypes=(torch.float32,), *, loose=False, width=None):
    """Check a [rows][ld] matrix with contiguous rows and return its row stride.  Two conventions:
    strict (score / attr / diag): every matrix with rows needs unit column stride, and one without
    rows has the stride ``width`` (default: its own width);  ``loose`` (kmeans / term_ce): a
    one-column matrix may have any column stride, and a single row's stride is at least its width."""
    if t.dim() != 2 or t.dtype not in dtypes or ((t.shape[1] > 1 if loose else t.shape[0]) and t.stride(1) != 1):
        raise ValueError(f"{what} is a {' / '.join(str(d) for d in dtypes)} [rows][ld] matrix with contiguous rows")
    if loose:
        return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], t.stride(0))
    return t.stride(0) if t.shape[0] else (t.shape[1] if width is None else int(width))


def _per_row(t, what, name, dtype, rows):
    """One value per row: ``t`` on the device, flattened, as contiguous ``dtype`` [rows]."""
    L.require_device(t, what)
    t = t.reshape(-1).to(dtype).contiguous()
    if t.numel() != rows:
        raise ValueError(f"{what}: one {name} per row ({rows} rows)")
    return t


def _dev_tensor(t, dtype, numel, what):
    if t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or t.numel() != numel:
        raise ValueError(f"{what} is a contiguous device {dtype} of {numel} elements")
    return t.data_ptr()


def gemm(a, b, *, a_kcontig=True, b_kcontig=True, M=None, N=None, K=None, out=None, out_dtype=None,
         bias=None, resid=None, epilogue=0, aux=None, aux_out=None, alpha=1.0, drop_seed=0, drop_p=0.0,
         split_k=1, colsum_out=None, n_valid=0, rope=None, tile=0, max_wg=0):
    """C[m,n] = epi(alpha * sum_k A(m,k) B(n,k)); A(m,k)=a[m,k] if a_kcontig else a[k,m]; same for B.
    colsum_out (fp32 [N]): also the column sums of C (CG_EPI_COLSUM partials + cg_colsum_reduce).
    rope = (cos, sin, T, hd, heads): CG_EPI_ROPE -- the first heads*hd columns rotated at position
    m % T after the bias (tables fp32 [>= T][hd/2]).  tile: L.TILE_* (0 = automatic); max_wg: cap
    on the persistent grid (0 = one workgroup per CU)."""
    for t in (a, b):
        L.require_device(t, "gemm")
    if a.dtype != b.dtype:
        raise ValueError("a and b must share a dtype")
    if M is None:
        M = a.shape[0] if a_kcontig else a.shape[1]
    if K is None:
        K = a.shape[1] if a_kcontig else a.shape[0]
    if N is None:
        N = b.shape[0] if b_kcontig else b.shape[1]
    out_dtype = out_dtype or (out.dtype if out is not None else a.dtype)
    if out is None:
        out = torch.empty(M, N, dtype=out_dtype, device=a.device)
    ws = None
    if split_k > 1:
        ws = torch.empty(split_k * M * N, dtype=torch.float32, device=a.device)
    if colsum_out is not None:
        if split_k > 1:
            raise ValueError("colsum_out needs split_k == 1")
        epilogue = int(epilogue) | L.EPI_COLSUM
        ws = torch.empty(((M + 63) // 64) * N, dtype=torch.float32, device=a.device)
    d = L.GemmDesc()
    d.in_dtype, d.c_dtype = _dt(a), _dt(out)
    d.M, d.N, d.K = M, N, K
    d.A, d.lda, d.a_kcontig = a.data_ptr(), a.stride(0), int(a_kcontig)
    d.B, d.ldb, d.b_kcontig = b.data_ptr(), b.stride(0), int(b_kcontig)
    d.C, d.ldc = out.data_ptr(), out.stride(0)
    d.epilogue = int(epilogue)
    d.alpha = float(alpha)
    d.bias = _p(bias)
    d.resid, d.ldr = _p(resid), (resid.stride(0) if resid is not None else 0)
    d.aux = _p(aux)
    d.aux_out = _p(aux_out)
    aux_t = aux if aux is not None else aux_out
    d.ld_aux = aux_t.stride(0) if aux_t is not None else 0
    d.drop_seed, d.drop_p = int(drop_seed) & 0xFFFFFFFF, float(drop_p)
    d.split_k = int(split_k)
    if ws is not None:
        _set_ws(d, ws)
    d.n_valid = int(n_valid)
    d.tile, d.max_wg = int(tile), int(max_wg)
    if rope is not None:
        cos, sin, rT, rhd, rheads = rope
        d.epilogue |= L.EPI_ROPE
        d.rope_cos, d.rope_sin = cos.data_ptr(), sin.data_ptr()
        d.rope_T, d.rope_hd, d.rope_heads = int(rT), int(rhd), int(rheads)
    L.check(L.lib.cg_gemm(C.byref(d), L.stream_ptr(a.device)), "cg_gemm")
    if colsum_out is not None:
        L.check(L.lib.cg_colsum_reduce(ws.data_ptr(), (M + 63) // 64, N, colsum_out.data_ptr(), 0,
                                       L.stream_ptr(a.device)), "cg_colsum_reduce")
    return out


def _ln_fwd_outputs(x, out_dtype):
    """(rows, cols, y, mean, rstd) of a LayerNorm forward over x [rows][cols]."""
    rows, cols = x.shape
    y = torch.empty(rows, cols, dtype=out_dtype, device=x.device)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    return rows, cols, y, mean, torch.empty_like(mean)


def layernorm_fwd(x, weight, bias, out_dtype=torch.float32, eps=1e-5):
    L.require_device(x, "layernorm_fwd")
    rows, cols, y, mean, rstd = _ln_fwd_outputs(x, out_dtype)
    L.check(L.lib.cg_layernorm_fwd(_dt(y), x.data_ptr(), x.stride(0), weight.data_ptr(), bias.data_ptr(),
                                   y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(), rows, cols, eps,
                                   L.stream_ptr(x.device)), "cg_layernorm_fwd")
    return y, mean, rstd


def layernorm_fwd_mask(x, weight, bias, B, T, H, drop_seed, drop_p, out_dtype=torch.bfloat16, eps=1e-5):
    """cg_layernorm_fwd_mask: layernorm_fwd and the attention-dropout keep words (attn_drop_mask) in one
    launch -> (y, mean, rstd, mask)."""
    L.require_device(x, "layernorm_fwd_mask")
    rows, cols, y, mean, rstd = _ln_fwd_outputs(x, out_dtype)
    n = int(L.lib.cg_attn_drop_mask_bytes(B, T, H))
    mask = torch.zeros(max(n, 4) // 4, dtype=torch.int32, device=x.device)
    L.check(L.lib.cg_layernorm_fwd_mask(_dt(y), x.data_ptr(), x.stride(0), weight.data_ptr(), bias.data_ptr(),
                                        y.data_ptr(), y.stride(0), mean.data_ptr(), rstd.data_ptr(), rows, cols, eps,
                                        B, T, H, int(drop_seed) & 0xFFFFFFFF, float(drop_p), mask.data_ptr(),
                                        L.stream_ptr(x.device)), "cg_layernorm_fwd_mask")
    return y, mean, rstd, mask


def layernorm_bwd(dy, x, mean, rstd, weight, g_in=None, eps=1e-5, branch_dtype=None, drop_seed=0, drop_p=0.0):
    """LayerNorm backward.  With `branch_dtype`, also returns the consumer-branch copy of g_out
    (dropout-masked with (drop_seed, drop_p)) and its column sums (the producing Linear's bias grad):
    (g_out, dgamma, dbeta, g_branch, colsum); else (g_out, dgamma, dbeta)."""
    rows, cols = x.shape
    g_out = torch.empty(rows, cols, dtype=torch.float32, device=x.device)
    part_bytes = int(L.lib.cg_layernorm_bwd_workspace(rows, cols, 1))
    part = torch.empty(max(1, part_bytes // 4), dtype=torch.float32, device=x.device)
    dgamma = torch.empty(cols, dtype=torch.float32, device=x.device)
    dbeta = torch.empty_like(dgamma)
    branch = colsum = None
    if branch_dtype is not None:
        branch = torch.empty(rows, cols, dtype=branch_dtype, device=x.device)
        colsum = torch.empty_like(dgamma)
    L.check(L.lib.cg_layernorm_bwd(_dt(dy), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), mean.data_ptr(),
                                   rstd.data_ptr(), weight.data_ptr(), _p(g_in), g_out.data_ptr(),
                                   _dt(branch) if branch is not None else L.CG_F32, _p(branch), drop_seed, drop_p,
                                   part.data_ptr(), part_bytes, dgamma.data_ptr(), dbeta.data_ptr(), _p(colsum), 0,
                                   rows, cols,
                                   eps, L.stream_ptr(x.device)), "cg_layernorm_bwd")
    if branch_dtype is not None:
        return g_out, dgamma, dbeta, branch, colsum
    return g_out, dgamma, dbeta


def layernorm_bwd_partials(dy, x, mean, rstd, weight, g_in=None, branch_dtype=None, drop_seed=0, drop_p=0.0):
    """LayerNorm backward row pass without the parameter reduction (cg_layernorm_bwd_partials):
    returns (g_out, partials [nblk][(2 + want_col) * cols], branch or None)."""
    rows, cols = x.shape
    g_out = torch.empty(rows, cols, dtype=torch.float32, device=x.device)
    nblk = L.lib.cg_layernorm_bwd_blocks(rows)
    nw = 3 if branch_dtype is not None else 2
    part = torch.empty(nblk, nw * cols, dtype=torch.float32, device=x.device)
    branch = torch.empty(rows, cols, dtype=branch_dtype, device=x.device) if branch_dtype is not None else None
    L.check(L.lib.cg_layernorm_bwd_partials(_dt(dy), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0),
                                            mean.data_ptr(), rstd.data_ptr(), weight.data_ptr(), _p(g_in),
                                            g_out.data_ptr(), _dt(branch) if branch is not None else L.CG_F32,
                                            _p(branch), drop_seed, drop_p, part.data_ptr(),
                                            _nbytes(part), int(nw == 3), rows, cols,
                                            L.stream_ptr(x.device)), "cg_layernorm_bwd_partials")
    return g_out, part, branch


def reduce_columns(jobs):
    """One cg_reduce_columns launch over jobs = [(part 2-D fp32 view, dst fp32 [cols], accumulate)]:
    dst (+)= part.sum(0) in the kernel's fixed order."""
    bt = L.ReduceBatch()
    bt.n = len(jobs)
    dev = None
    for i, (part, dst, acc) in enumerate(jobs):
        j = bt.j[i]
        j.part = part.data_ptr(); j.ld = part.stride(0); j.nrows = part.shape[0]; j.cols = part.shape[1]
        j.dst = dst.data_ptr(); j.accumulate = int(acc)
        dev = part.device
    L.check(L.lib.cg_reduce_columns(C.byref(bt), L.stream_ptr(dev) if dev is not None else None),
            "cg_reduce_columns")


def swiglu_fwd(gu, H):
    """s[:, j] = silu(gu[:, j]) * gu[:, Hp + j] for j < H (0 for H <= j < Hp), Hp = gu.shape[1] // 2."""
    rows, Hp = gu.shape[0], gu.shape[1] // 2
    s = torch.empty(rows, Hp, dtype=gu.dtype, device=gu.device)
    L.check(L.lib.cg_swiglu_fwd(_dt(gu), gu.data_ptr(), gu.stride(0), Hp, s.data_ptr(), s.stride(0), rows, H,
                                L.stream_ptr(gu.device)), "cg_swiglu_fwd")
    return s


def swiglu_bwd(gu, ds, H):
    """d(gate | up) of swiglu_fwd for the upstream gradient ds [rows][Hp]."""
    rows, Hp = gu.shape[0], gu.shape[1] // 2
    dgu = torch.empty_like(gu)
    L.check(L.lib.cg_swiglu_bwd(_dt(gu), gu.data_ptr(), gu.stride(0), Hp, ds.data_ptr(), ds.stride(0),
                                dgu.data_ptr(), dgu.stride(0), rows, H, L.stream_ptr(gu.device)), "cg_swiglu_bwd")
    return dgu


def rope_(qkv, B, T, H, KV, hd, cos_tab, sin_tab, inverse=False):
    """In-place rotate-half RoPE of the q and k heads of qkv [B*T][ld] (cos/sin fp32 [T][hd/2])."""
    L.check(L.lib.cg_rope_tab(_dt(qkv), qkv.data_ptr(), qkv.stride(0), B, T, H, KV, hd, cos_tab.data_ptr(),
                              sin_tab.data_ptr(), int(inverse), L.stream_ptr(qkv.device)), "cg_rope_tab")
    return qkv


def segment_starts(idx, sep_id):
    B, T = idx.shape
    out = torch.empty(B, T, dtype=torch.int32, device=idx.device)
    L.check(L.lib.cg_segment_starts(idx.contiguous().data_ptr(), out.data_ptr(), B, T,
                                    -1 if sep_id is None else int(sep_id), L.stream_ptr(idx.device)),
            "cg_segment_starts")
    return out


def attn_drop_mask(B, T, H, drop_seed, drop_p, device):
    """Attention-dropout keep bits (query-major + key-major words) for cg_attn_fwd / cg_attn_bwd."""
    n = int(L.lib.cg_attn_drop_mask_bytes(B, T, H))
    mask = torch.empty(max(n, 4) // 4, dtype=torch.int32, device=device)
    L.check(L.lib.cg_attn_drop_mask(B, T, H, int(drop_seed) & 0xFFFFFFFF, float(drop_p), mask.data_ptr(),
                                    L.stream_ptr(device)), "cg_attn_drop_mask")
    return mask


def attn_fwd(qkv, segstart, B, T, H, KV, hd, window=0, drop_seed=0, drop_p=0.0, drop_mask=None):
    y = torch.empty(B * T, H * hd, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B * H * T, dtype=torch.float32, device=qkv.device)
    L.check(L.lib.cg_attn_fwd(_dt(qkv), qkv.data_ptr(), qkv.stride(0), _p(segstart), y.data_ptr(), y.stride(0),
                              lse.data_ptr(), B, T, H, KV, hd, int(window or 0), int(drop_seed) & 0xFFFFFFFF,
                              float(drop_p), _p(drop_mask), L.stream_ptr(qkv.device)), "cg_attn_fwd")
    return y, lse


def attn_fwd_keep(qkv, segstart, B, T, H, KV, hd, drop_seed, drop_p, window=0, mask=None):
    """Dropout forward that also writes the keep bits for the backward (cg_attn_fwd_keep): (y, lse, mask).
    `mask` (optional): the cg_attn_drop_mask_bytes buffer to write into."""
    if mask is None:
        n = int(L.lib.cg_attn_drop_mask_bytes(B, T, H))
        mask = torch.zeros(max(n, 4) // 4, dtype=torch.int32, device=qkv.device)
    y = torch.empty(B * T, H * hd, dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty(B * H * T, dtype=torch.float32, device=qkv.device)
    L.check(L.lib.cg_attn_fwd_keep(_dt(qkv), qkv.data_ptr(), qkv.stride(0), _p(segstart), y.data_ptr(), y.stride(0),
                                   lse.data_ptr(), B, T, H, KV, hd, int(window or 0), int(drop_seed) & 0xFFFFFFFF,
                                   float(drop_p), mask.data_ptr(), L.stream_ptr(qkv.device)), "cg_attn_fwd_keep")
    return y, lse, mask


ATTN_BWD_ALGO = {None: 0, "auto": 0, "split": 1, "fused": 2}


def attn_bwd(qkv, segstart, y, dy, lse, B, T, H, KV, hd, window=0, drop_seed=0, drop_p=0.0, drop_mask=None,
             bias_part=None, rope=None, algo=None):
    """dqkv; with bias_part (fp32 [B*ceil(T/128)][ld >= (H+2KV) hd], bf16 MFMA path) also the per-tile
    column sums of dqkv that cg_colsum_reduce turns into the q/k/v bias gradients.  rope = (cos, sin)
    fp32 [T][hd/2] tables: qkv holds rotated q / k and dQ / dK come back w.r.t. the un-rotated ones
    (cg_attn_bwd_rope, bf16 MFMA path).  algo: None / "auto", "split" (dQ kernel + dK/dV kernel) or
    "fused" (one pass, cg_attn_bwd_algo) for the bf16 MFMA backward."""
    dqkv = torch.zeros_like(qkv)
    ws = torch.empty(int(L.lib.cg_attn_bwd_workspace(B, T, H)) // 4 + 1, dtype=torch.float32, device=qkv.device)
    args = [_dt(qkv), qkv.data_ptr(), qkv.stride(0), _p(segstart), y.data_ptr(), y.stride(0), dy.data_ptr(),
            dy.stride(0), lse.data_ptr(), dqkv.data_ptr(), dqkv.stride(0), B, T, H, KV, hd, int(window or 0),
            int(drop_seed) & 0xFFFFFFFF, float(drop_p), _p(drop_mask), _p(bias_part),
            0 if bias_part is None else bias_part.stride(0)]
    tail = [ws.data_ptr(), _nbytes(ws), L.stream_ptr(qkv.device)]
    if algo is not None:
        rp = [None, None] if rope is None else [rope[0].data_ptr(), rope[1].data_ptr()]
        L.check(L.lib.cg_attn_bwd_algo(ATTN_BWD_ALGO[algo], *args, *rp, *tail), "cg_attn_bwd_algo")
    elif rope is None:
        L.check(L.lib.cg_attn_bwd(*args, *tail), "cg_attn_bwd")
    else:
        L.check(L.lib.cg_attn_bwd_rope(*args, rope[0].data_ptr(), rope[1].data_ptr(), *tail), "cg_attn_bwd_rope")
    return dqkv


def cross_entropy(logits, targets, eps=0.0, weight=None, ignore_index=0, grad_dtype=torch.float32, pad_to=None,
                  grad_scale=1.0, split=False):
    """(loss, dlogits [rows][pad_to or V]); the gradient is multiplied by grad_scale, the loss is not.
    split (CG_BF16X2): dlogits is bf16 [rows][pad_to], hi = bf16(g) at column c and lo = bf16(g - hi)
    at column pad_to/2 + c (pad_to even, pad_to/2 >= V)."""
    rows, V = logits.shape
    ldd = pad_to or V
    if split:
        grad_dtype = torch.bfloat16
    dl = torch.empty(rows, ldd, dtype=grad_dtype, device=logits.device)
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    ws = torch.empty(int(L.lib.cg_ce_workspace(rows)) // 4 + 1, dtype=torch.float32, device=logits.device)
    L.check(L.lib.cg_cross_entropy(logits.data_ptr(), logits.stride(0), targets.contiguous().data_ptr(), rows, V,
                                   float(eps), _p(weight), int(ignore_index), float(grad_scale),
                                   L.CG_BF16X2 if split else _dt(dl), dl.data_ptr(), ldd,
                                   loss.data_ptr(), ws.data_ptr(), _nbytes(ws), L.stream_ptr(logits.device)),
            "cg_cross_entropy")
    return loss, dl


def adamw_(param, grad, exp_avg, exp_avg_sq, step, segments, shadow=None, beta1=0.9, beta2=0.999, eps=1e-8,
           grad_scale=1.0):
    """In-place AdamW over flat fp32 buffers; segments: [(begin, end, lr, wd)]."""
    n = len(segments)
    segs = (L.AdamwSegment * n)()
    for i, (b, e, lr, wd) in enumerate(segments):
        segs[i].begin, segs[i].end, segs[i].lr, segs[i].wd = int(b), int(e), float(lr), float(wd)
    L.check(L.lib.cg_adamw(param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                           _p(shadow), segs, n, beta1, beta2, eps, int(step), float(grad_scale),
                           L.stream_ptr(param.device)), "cg_adamw")


def cast_to_bf16(x):
    out = torch.empty(x.numel(), dtype=torch.bfloat16, device=x.device)
    L.check(L.lib.cg_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), x.numel(), L.stream_ptr(x.device)),
            "cg_cast_f32_to_bf16")
    return out.view(x.shape)


def cast_from_bf16(x):
    """bf16 -> fp32 (exact), any shape."""
    L.require_device(x, "cast_from_bf16")
    if x.dtype != torch.bfloat16 or not x.is_contiguous():
        raise ValueError("cast_from_bf16 takes a contiguous bf16 tensor")
    out = torch.empty(x.numel(), dtype=torch.float32, device=x.device)
    L.check(L.lib.cg_cast_bf16_to_f32(x.data_ptr(), out.data_ptr(), x.numel(), L.stream_ptr(x.device)),
            "cg_cast_bf16_to_f32")
    return out.view(x.shape)


def cast_pad_2d(src, dcols, dtype=torch.bfloat16, out=None, split=False):
    """fp32 [rows][cols] -> dtype [rows][dcols], pad columns zero.  split (CG_BF16X2): bf16
    [rows][2 dcols], hi = bf16(v) at column c and lo = bf16(v - hi) at column dcols + c.
    out (optional): the destination, a row-major view at least that wide (its row stride is used)."""
    L.require_device(src, "cast_pad_2d")
    rows, cols = src.shape
    if split:
        dtype = torch.bfloat16
    if out is None:
        out = torch.empty(rows, 2 * dcols if split else dcols, dtype=dtype, device=src.device)
    elif out.dtype != dtype or out.dim() != 2 or out.shape[0] != rows or out.stride(1) != 1:
        raise ValueError("cast_pad_2d: out must be a row-major [rows][*] view of the destination dtype")
    L.check(L.lib.cg_cast_pad_2d(src.data_ptr(), src.stride(0), rows, cols, L.CG_BF16X2 if split else _dt(out),
                                 out.data_ptr(), out.stride(0), dcols, L.stream_ptr(src.device)), "cg_cast_pad_2d")
    return out


def scale_dev_(x, scale, cols=None, split=False):
    """In-place x[:, :cols] *= scale[()] with the scale read on the device (fp32 scalar tensor).
    x: row-major 2-D fp32 / bf16 view (row stride = ld).  split (CG_BF16X2): bf16 rows holding
    hi in [0, ld/2) and lo in [ld/2, ld); the pair sum is scaled and split again."""
    L.require_device(x, "scale_dev_")
    L.require_device(scale, "scale_dev_")
    if x.dim() != 2 or x.stride(1) != 1 or scale.dtype != torch.float32:
        raise ValueError("scale_dev_: row-major 2-D x and an fp32 device scalar")
    rows = x.shape[0]
    if cols is None:
        cols = x.shape[1] // 2 if split else x.shape[1]
    L.check(L.lib.cg_scale_dev(L.CG_BF16X2 if split else _dt(x), x.data_ptr(), x.stride(0), rows, int(cols),
                               scale.data_ptr(), L.stream_ptr(x.device)), "cg_scale_dev")
    return x


def nonfinite_flag(x, flag=None):
    """flag (int32 device scalar, created zero when None) |= any(!isfinite(x)) over a contiguous fp32 x."""
    L.require_device(x, "nonfinite_flag")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("nonfinite_flag takes a contiguous fp32 tensor")
    if flag is None:
        flag = torch.zeros((), dtype=torch.int32, device=x.device)
    L.check(L.lib.cg_nonfinite_flag(x.data_ptr(), x.numel(), flag.data_ptr(), L.stream_ptr(x.device)),
            "cg_nonfinite_flag")
    return flag


def embed_fwd(idx, tok_emb, pos_emb=None, drop_seed=0, drop_p=0.0, out=None):
    """x[b*T + t] = dropout(tok_emb[idx[b, t]] (+ pos_emb[t])) as fp32 [B*T][d] (keep bits
    cg_keep(seed, row, column)).  out (optional): a contiguous fp32 [B*T][d] destination."""
    L.require_device(idx, "embed_fwd")
    L.require_device(tok_emb, "embed_fwd")
    B, T = idx.shape
    d = tok_emb.shape[1]
    if idx.dtype != torch.int64 or tok_emb.dtype != torch.float32 or not tok_emb.is_contiguous():
        raise ValueError("embed_fwd: int64 ids and a contiguous fp32 table")
    if pos_emb is not None and (pos_emb.dtype != torch.float32 or not pos_emb.is_contiguous()
                                or pos_emb.shape[0] < T or pos_emb.shape[1] != d):
        raise ValueError("embed_fwd: pos_emb must be a contiguous fp32 [>= T][d]")
    if out is None:
        out = torch.empty(B * T, d, dtype=torch.float32, device=tok_emb.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B * T, d) or not out.is_contiguous():
        raise ValueError("embed_fwd: out must be a contiguous fp32 [B*T][d]")
    L.check(L.lib.cg_embed_fwd(idx.contiguous().data_ptr(), tok_emb.data_ptr(), _p(pos_emb), out.data_ptr(), B, T, d,
                               int(drop_seed) & 0xFFFFFFFF, float(drop_p), L.stream_ptr(tok_emb.device)),
            "cg_embed_fwd")
    return out


def _decode_cache_check(what, q, cache, Tmax):
    """(B, Tmax) of a decode step's q [B][>= H hd] and KV cache [B][Tmax][ldc] (Tmax None = the cache's)."""
    if q.dtype != cache.dtype or cache.dim() != 3 or cache.stride(2) != 1 or q.stride(1) != 1:
        raise ValueError(f"{what}: q and cache share a dtype; cache is [B][Tmax][ldc]")
    B = q.shape[0]
    if Tmax is None:
        Tmax = cache.shape[1]
    if cache.shape[0] != B or cache.stride(0) != Tmax * cache.stride(1):
        raise ValueError(f"{what}: cache rows of one sequence must be Tmax consecutive rows")
    return B, Tmax


def attn_decode(q, cache, pos, H, KV, hd, segstate=None, window=0, Tmax=None):
    """One-token attention over a KV cache: q [B][>= H hd], cache [B][Tmax][ldc] (K head kvh at
    column kvh hd, V at KV hd + kvh hd); the query of position `pos` sees keys lo..pos, lo =
    segstate[b] (int32 [B], None = 0) raised to pos - window + 1 with a window -> y [B][H hd]."""
    L.require_device(q, "attn_decode")
    L.require_device(cache, "attn_decode")
    B, Tmax = _decode_cache_check("attn_decode", q, cache, Tmax)
    y = torch.empty(B, H * hd, dtype=q.dtype, device=q.device)
    L.check(L.lib.cg_attn_decode(_dt(q), q.data_ptr(), q.stride(0), cache.data_ptr(), cache.stride(1), int(Tmax),
                                 int(pos), _p(segstate), int(window or 0), B, H, KV, hd, y.data_ptr(), y.stride(0),
                                 L.stream_ptr(q.device)), "cg_attn_decode")
    return y


def attn_decode_ragged(q, cache, pos, H, KV, hd, segstate=None, window=0, Tmax=None, out=None):
    """cg_attn_decode_ragged: attn_decode with one position per sequence, pos int32 [B] on the
    device; rows with pos < 0 or >= Tmax are inactive and keep their row of ``out`` (zeros when
    ``out`` is not given)."""
    L.require_device(q, "attn_decode_ragged")
    L.require_device(cache, "attn_decode_ragged")
    L.require_device(pos, "attn_decode_ragged")
    B, Tmax = _decode_cache_check("attn_decode_ragged", q, cache, Tmax)
    if pos.dtype != torch.int32 or pos.numel() != B or not pos.is_contiguous():
        raise ValueError("attn_decode_ragged: pos is a contiguous int32 [B]")
    y = out if out is not None else torch.zeros(B, H * hd, dtype=q.dtype, device=q.device)
    L.check(L.lib.cg_attn_decode_ragged(_dt(q), q.data_ptr(), q.stride(0), cache.data_ptr(), cache.stride(1),
                                        int(Tmax), pos.data_ptr(), _p(segstate), int(window or 0), B, H, KV, hd,
                                        y.data_ptr(), y.stride(0), L.stream_ptr(q.device)), "cg_attn_decode_ragged")
    return y


def _sample_args_check(what, logits, state, next_tok, out_ids):
    """B of a sampling step's device tensors: logits fp32 [B][V], state int32 [B][8], int64 ids."""
    for t in (logits, state, next_tok, out_ids):
        L.require_device(t, what)
    B = logits.shape[0]
    if (logits.dtype != torch.float32 or state.dtype != torch.int32 or tuple(state.shape) != (B, 8)
            or not state.is_contiguous() or next_tok.dtype != torch.int64 or out_ids.dtype != torch.int64):
        raise ValueError(f"{what}: logits fp32 [B][V], state int32 [B][8], next_tok / out_ids int64")
    return B


def sample_step(params, logits, state, next_tok, out_ids, n_active=None, term_logits=None):
    """cg_sample_step in place: ``params`` a _lib.SampleParams, logits fp32 [B][V], state int32 [B][8]
    (cg_gen_state rows), next_tok int64 [B], out_ids int64 [B][cap], n_active int32 [1]."""
    B = _sample_args_check("sample_step", logits, state, next_tok, out_ids)
    L.check(L.lib.cg_sample_step(C.byref(params), logits.data_ptr(), logits.stride(0), _p(term_logits),
                                 term_logits.stride(0) if term_logits is not None else 0, state.data_ptr(),
                                 next_tok.data_ptr(), out_ids.data_ptr(), out_ids.stride(0), _p(n_active), B,
                                 L.stream_ptr(logits.device)), "cg_sample_step")


def sample_step_plan(params, plan, logits, state, next_tok, out_ids, n_active=None, term_logits=None):
    """cg_sample_step_plan in place: sample_step's arguments plus ``plan``, a _lib.SamplePlan whose
    pointers the caller keeps alive (sets uint8 [n_sets][ld_sets], plan int32 [B][ld_plan], plan_len
    int32 [B], logp fp64 [B][2], tok_logp fp32 [B][ld_tok_logp])."""
    B = _sample_args_check("sample_step_plan", logits, state, next_tok, out_ids)
    L.check(L.lib.cg_sample_step_plan(C.byref(params), C.byref(plan) if plan is not None else None,
                                      logits.data_ptr(), logits.stride(0), _p(term_logits),
                                      term_logits.stride(0) if term_logits is not None else 0, state.data_ptr(),
                                      next_tok.data_ptr(), out_ids.data_ptr(), out_ids.stride(0), _p(n_active), B,
                                      L.stream_ptr(logits.device)), "cg_sample_step_plan")


def gather_rows(src, sel, T):
    """cg_gather_rows with T > 0: out[b] = src[b*T + sel[b] - 1] for fp32 src [B*T][n] and a device
    int32 sel [B] of 1-based row counts (sel = T picks every sequence's last row)."""
    L.require_device(src, "gather_rows")
    if src.dim() != 2 or src.dtype != torch.float32 or src.stride(1) != 1 or T <= 0 or src.shape[0] % T:
        raise ValueError("gather_rows: src is fp32 [B*T][n]")
    B, n = src.shape[0] // T, src.shape[1]
    if sel.dtype != torch.int32 or sel.numel() != B or not sel.is_cuda or not sel.is_contiguous():
        raise ValueError("gather_rows: sel is a contiguous device int32 [B]")
    out = torch.empty(B, n, dtype=torch.float32, device=src.device)
    L.check(L.lib.cg_gather_rows(src.data_ptr(), src.stride(0), sel.data_ptr(), int(T), int(T), out.data_ptr(), n, n,
                                 None, None, B, L.stream_ptr(src.device)), "cg_gather_rows")
    return out


class ScoreResult(_Result):
    """Device tensors of one score_rows call; an output that was not asked for is None."""
    __slots__ = ("lse", "logp", "entropy", "argmax", "rank", "delta", "seq_logp", "seq_count", "acc")


SCORE_OUTPUTS = ("lse", "logp", "entropy", "argmax", "rank", "delta", "seq_logp", "seq_count")


def score_workspace(rows, device):
    """A cg_score_rows workspace for up to ``rows`` rows (8-byte aligned)."""
    return _alloc_ws(L.lib.cg_score_workspace(int(rows)), device, "f64")


def score_rows(logits, targets=None, *, V=None, ignore_index=0, smoothing=0.0, sel=None, T=0, acc=None,
               want=("lse", "logp", "entropy", "argmax", "rank"), workspace=None):
    """cg_score_rows over fp32 logits [rows][ld] (only the first ``V`` columns of a row are read):
    a ScoreResult with the row outputs named in ``want`` (fp32 lse / logp / entropy, int32 argmax /
    rank), ``delta`` fp32 [rows][len(sel)] for the device int32 class list ``sel``, ``seq_logp``
    fp64 [rows / T] and ``seq_count`` int32 with ``T`` rows per sequence, and ``acc``: the fp64 [4]
    accumulator the launch added to (nll sum, smoothed sum, valid rows, top-1 hits)."""
    L.require_device(logits, "score_rows")
    ldl = _row_matrix(logits, "score_rows: logits", width=V)
    _check_want("score_rows", want, SCORE_OUTPUTS)
    rows = logits.shape[0]
    V = logits.shape[1] if V is None else int(V)
    dev = logits.device
    d = L.ScoreDesc()
    d.logits, d.ldl, d.rows, d.V = logits.data_ptr(), ldl, rows, V
    if targets is not None:
        targets = _per_row(targets, "score_rows", "target", torch.int64, rows)
        d.targets = targets.data_ptr()
    d.ignore_index, d.smoothing, d.T = int(ignore_index), float(smoothing), int(T)
    res = ScoreResult()
    if "delta" in want or sel is not None:
        if sel is None or sel.dtype != torch.int32 or not sel.is_cuda or not sel.is_contiguous() or sel.numel() < 1:
            raise ValueError("score_rows: delta needs sel, a contiguous device int32 class list")
        res.delta = torch.empty(rows, sel.numel(), dtype=torch.float32, device=dev)
        d.sel, d.n_sel, d.delta, d.ld_delta = sel.data_ptr(), sel.numel(), res.delta.data_ptr(), sel.numel()
    if ("seq_logp" in want or "seq_count" in want) and (T <= 0 or rows % T):
        raise ValueError("score_rows: sequence sums need T > 0 dividing the row count")
    seqs = rows // T if T > 0 else 0
    _alloc_outputs(d, res, want, dev, (
        ("lse", rows, torch.float32), ("logp", rows, torch.float32), ("entropy", rows, torch.float32),
        ("argmax", rows, torch.int32), ("rank", rows, torch.int32),
        ("seq_logp", seqs, torch.float64), ("seq_count", seqs, torch.int32)))
    if acc is not None:
        res.acc, d.acc = acc, _dev_tensor(acc, torch.float64, 4, "score_rows: acc")
    _set_ws(d, _pick_ws(workspace, dev, "f64", False, L.lib.cg_score_workspace, rows))
    L.check(L.lib.cg_score_rows(C.byref(d), L.stream_ptr(dev)), "cg_score_rows")
    return res


ATTR_MODES = {"logprob": L.ATTR_LOGPROB, "logit": L.ATTR_LOGIT}


def attr_seed(logits, y, w=None, *, V=None, mode="logprob", pad_to=None, split=False):
    """cg_attr_seed over fp32 logits [rows][ld] (the first ``V`` columns of a row are read): the
    gradient of sum_r w[r] log p(y[r]) (``mode`` "logprob") or of sum_r w[r] z[r][y[r]] ("logit")
    with respect to the logits, fp32 [rows][pad_to or V] -- or, with ``split`` (CG_BF16X2), bf16
    [rows][pad_to] with hi at column c and lo at column pad_to/2 + c (pad_to even, pad_to/2 >= V).
    ``y`` int64 [rows] and ``w`` fp32 [rows] (None = 1) live on the device; a row with y outside
    [0, V) or w == 0 is all zero, and so are the pad columns."""
    L.require_device(logits, "attr_seed")
    ldl = _row_matrix(logits, "attr_seed: logits", width=V)
    if mode not in ATTR_MODES:
        raise ValueError(f"attr_seed: mode is one of {sorted(ATTR_MODES)}")
    rows = logits.shape[0]
    V = logits.shape[1] if V is None else int(V)
    dev = logits.device
    y = _per_row(y, "attr_seed", "class", torch.int64, rows)
    if w is not None:
        w = _per_row(w, "attr_seed", "weight", torch.float32, rows)
    ldd = int(pad_to) if pad_to else (2 * V if split else V)
    out = torch.empty(rows, ldd, dtype=torch.bfloat16 if split else torch.float32, device=dev)
    L.check(L.lib.cg_attr_seed(logits.data_ptr(), ldl, y.data_ptr(), _p(w), rows, V,
                               ATTR_MODES[mode], L.CG_BF16X2 if split else L.CG_F32, out.data_ptr(), ldd,
                               L.stream_ptr(dev)), "cg_attr_seed")
    return out


class AttrResult(_Result):
    """Device tensors of one attr_reduce / Engine.input_grad call; an output that was not asked for
    is None."""
    __slots__ = ("gxt", "gxi", "gnorm", "dx0")


ATTR_OUTPUTS = ("gxt", "gxi", "gnorm")


def attr_reduce(g, idx, tok_emb=None, x0=None, *, want=ATTR_OUTPUTS):
    """cg_attr_reduce of an input gradient ``g`` fp32 [rows][d] (row stride >= d): an AttrResult with
    ``gxt`` = g . tok_emb[idx] (0 where idx is outside the table), ``gxi`` = g . x0 and ``gnorm`` =
    |g|, fp32 [rows] each, for the outputs named in ``want``.  ``idx`` int64 [rows], ``tok_emb`` fp32
    [V][>= d] and ``x0`` fp32 [rows][>= d] live on the device."""
    L.require_device(g, "attr_reduce")
    _check_want("attr_reduce", want, ATTR_OUTPUTS)
    ldg = _row_matrix(g, "attr_reduce: g")
    for name, t in (("tok_emb", tok_emb), ("x0", x0)):  # their strides below: x0's follows g's row count
        if t is not None:
            _row_matrix(t, f"attr_reduce: {name}")
    rows, d = g.shape
    idx = _per_row(idx, "attr_reduce", "token id", torch.int64, rows)
    if "gxt" in want and (tok_emb is None or tok_emb.shape[1] != d):
        raise ValueError("attr_reduce: gxt needs tok_emb [V][d]")
    if "gxi" in want and (x0 is None or tuple(x0.shape) != (rows, d)):
        raise ValueError("attr_reduce: gxi needs x0 [rows][d]")
    res = AttrResult()
    _alloc_outputs(None, res, want, g.device, [(name, rows, torch.float32) for name in ATTR_OUTPUTS])
    L.check(L.lib.cg_attr_reduce(g.data_ptr(), ldg, idx.data_ptr(), _p(tok_emb),
                                 tok_emb.stride(0) if tok_emb is not None else 0,
                                 tok_emb.shape[0] if tok_emb is not None else 0, _p(x0),
                                 x0.stride(0) if x0 is not None and rows else d, rows, d, _p(res.gxt), _p(res.gxi),
                                 _p(res.gnorm), L.stream_ptr(g.device)), "cg_attr_reduce")
    return res


def attn_probs(qkv, segstart, lse, B, T, H, KV, hd, window=0):
    """softmax(QK^T / sqrt(hd)) on the visible (query, key) pairs from the forward's qkv rows and
    LSE, 0 elsewhere: fp32 [B][H][T][T]."""
    L.require_device(qkv, "attn_probs")
    out = torch.empty(B, H, T, T, dtype=torch.float32, device=qkv.device)
    L.check(L.lib.cg_attn_probs(_dt(qkv), qkv.data_ptr(), qkv.stride(0), _p(segstart), lse.data_ptr(), out.data_ptr(),
                                B, T, H, KV, hd, int(window or 0), L.stream_ptr(qkv.device)), "cg_attn_probs")
    return out


def segstate_step(tok, sep_id, pos, segstate):
    """In place: segstate[b] = pos where tok[b] == sep_id (sep_id None / negative: untouched)."""
    L.require_device(tok, "segstate_step")
    if tok.dtype != torch.int64 or segstate.dtype != torch.int32 or tok.numel() != segstate.numel():
        raise ValueError("segstate_step: int64 tokens [B], int32 state [B]")
    L.check(L.lib.cg_segstate_step(tok.contiguous().data_ptr(), tok.numel(), -1 if sep_id is None else int(sep_id),
                                   int(pos), segstate.data_ptr(), L.stream_ptr(tok.device)), "cg_segstate_step")
    return segstate


def _ids(values):
    vals = [int(v) for v in values]
    return (C.c_int * max(1, len(vals)))(*vals), len(vals)


def offset_targets(y, offset, boundary_ids=(2, 3), count=True):
    """(targets, n_valid): y[:, t+k-1] where offset_target_mask is true, else PAD (0).
    n_valid is a device int32 scalar (None with count=False)."""
    L.require_device(y, "offset_targets")
    y = y.to(torch.int64).contiguous()
    B, T = y.shape
    out = torch.empty_like(y)
    nv = torch.zeros((), dtype=torch.int32, device=y.device) if count else None
    ids, n = _ids(boundary_ids)
    L.check(L.lib.cg_offset_targets(y.data_ptr(), B, T, int(offset), ids, n, out.data_ptr(), _p(nv),
                                    L.stream_ptr(y.device)), "cg_offset_targets")
    return out, nv


def termination_labels(y, stop_ids, bucket_edges=(0, 3, 10, 30), ignore_index=-100):
    L.require_device(y, "termination_labels")
    y = y.to(torch.int64).contiguous()
    B, T = y.shape
    out = torch.empty_like(y)
    st, ns = _ids(stop_ids)
    ed, ne = _ids(bucket_edges)
    L.check(L.lib.cg_termination_labels(y.data_ptr(), B, T, st, ns, ed, ne, int(ignore_index), out.data_ptr(),
                                        L.stream_ptr(y.device)), "cg_termination_labels")
    return out


POOL_MODES = {"mean_nonpad": 0, "mean_content": 1, "eos": 2}


def pool_hidden(hidden, idx, mode, content_ids=(), pad_id=0):
    """_pool_state (extract_embeddings.py:94-114) of hidden (B, T, d) -> fp32 (B, d)."""
    L.require_device(hidden, "pool_hidden")
    B, T, d = hidden.shape
    if hidden.stride(2) != 1 or hidden.stride(0) != T * hidden.stride(1):
        hidden = hidden.contiguous()
    idx = idx.to(device=hidden.device, dtype=torch.int64).contiguous()
    mask = _id_mask(content_ids, "content ids")
    out = torch.empty(B, d, dtype=torch.float32, device=hidden.device)
    L.check(L.lib.cg_pool_hidden(_dt(hidden), hidden.data_ptr(), hidden.stride(1), idx.data_ptr(), B, T, d,
                                 int(pad_id), POOL_MODES[mode], mask, out.data_ptr(),
                                 L.stream_ptr(hidden.device)), "cg_pool_hidden")
    return out


def colsum(x, out=None, accumulate=False):
    """out[n] (+)= sum_m x[m, n] (fp32 out)."""
    L.require_device(x, "colsum")
    rows, cols = x.shape
    if out is None:
        out = torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(L.lib.cg_colsum_workspace(rows, cols)) // 4 + 1, dtype=torch.float32, device=x.device)
    L.check(L.lib.cg_colsum(_dt(x), x.data_ptr(), x.stride(0), rows, cols, out.data_ptr(), int(bool(accumulate)),
                            ws.data_ptr(), _nbytes(ws), L.stream_ptr(x.device)), "cg_colsum")
    return out


def transpose16(mats):
    """Batched transpose of 2-byte 2-D tensors (one launch); returns the contiguous transposes."""
    if len(mats) > L.TRANSPOSE_MAX:
        raise ValueError("too many matrices")
    tb = L.TransposeBatch()
    tb.n = len(mats)
    outs = []
    for i, m in enumerate(mats):
        if m.element_size() != 2 or m.dim() != 2 or m.stride(1) != 1:
            raise ValueError("transpose16 takes row-major 2-byte matrices")
        L.require_device(m, "transpose16")
        o = torch.empty(m.shape[1], m.shape[0], dtype=m.dtype, device=m.device)
        tb.items[i] = L.TransposeItem(m.data_ptr(), o.data_ptr(), m.stride(0), o.stride(0), m.shape[0], m.shape[1])
        outs.append(o)
    if mats:
        L.check(L.lib.cg_transpose16_batch(C.byref(tb), L.stream_ptr(mats[0].device)), "cg_transpose16_batch")
    return outs


def gemm_dw_grouped(products, *, tile_m=0, ksplit=1, max_wg=0, workspace=None):
    """Grouped weight gradients: for each (dy [K, N_out] bf16, x [K, K_out] bf16, out fp32
    [N_out, K_out], alpha, accumulate[, col_sum]) -> out (+)= alpha * dy^T x, one persistent launch
    (cg_gemm_dw_grouped).  Row strides are taken from the tensors.  ksplit > 1: each tile's K rows
    split over that many workgroups (fp32 slabs + one in-order reduction).  col_sum (fp32 [N_out],
    optional): (+)= alpha * the column sums of dy (the bias gradient), ksplit 1 only.  max_wg > 0
    caps the persistent grid (0: one workgroup per CU); workspace (fp32, ksplit > 1): the caller's
    slab buffer instead of a fresh one."""
    if not products:
        return
    if len(products) > L.DW_MAX:
        raise ValueError(f"at most {L.DW_MAX} products per group")
    g = L.DwGroup()
    g.n, g.tile_m, g.max_wg = len(products), int(tile_m), int(max_wg)
    K = None
    for i, (dy, x, out, alpha, acc, *cs) in enumerate(products):
        for t in (dy, x, out):
            L.require_device(t, "gemm_dw_grouped")
        if dy.dtype != torch.bfloat16 or x.dtype != torch.bfloat16 or out.dtype != torch.float32:
            raise ValueError("gemm_dw_grouped: bf16 operands, fp32 output")
        if K is None:
            K = dy.shape[0]
        if dy.shape[0] != K or x.shape[0] != K:
            raise ValueError("gemm_dw_grouped: every product reduces over the same K rows")
        p = g.p[i]
        p.A, p.lda, p.B, p.ldb = dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0)
        p.C, p.ldc = out.data_ptr(), out.stride(0)
        p.N_out, p.K_out = dy.shape[1], x.shape[1]
        if tuple(out.shape) != (p.N_out, p.K_out):
            raise ValueError("gemm_dw_grouped: out must be [N_out, K_out]")
        p.alpha, p.accumulate = float(alpha), int(bool(acc))
        if cs and cs[0] is not None:
            L.require_device(cs[0], "gemm_dw_grouped")
            if cs[0].dtype != torch.float32 or cs[0].numel() != p.N_out or not cs[0].is_contiguous():
                raise ValueError("gemm_dw_grouped: col_sum must be a contiguous fp32 [N_out]")
            p.col_sum = cs[0].data_ptr()
    g.K = int(K)
    ws = None
    if ksplit > 1:
        g.ksplit = int(ksplit)
        nbytes = int(L.lib.cg_gemm_dw_grouped_workspace(C.byref(g)))
        ws = workspace
        if ws is None:
            ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=products[0][0].device)
        elif ws.dtype != torch.float32 or not ws.is_contiguous() or _nbytes(ws) < nbytes:
            raise ValueError(f"gemm_dw_grouped: workspace must be contiguous fp32 of at least {nbytes} bytes")
        else:
            L.require_device(ws, "gemm_dw_grouped")
        _set_ws(g, ws)
    L.check(L.lib.cg_gemm_dw_grouped(C.byref(g), L.stream_ptr(products[0][0].device)), "cg_gemm_dw_grouped")
    return ws


def _id_mask(ids, what):
    words = [0] * 8
    for t in ids:
        t = int(t)
        if not 0 <= t < 256:
            raise ValueError(f"{what} must be in [0, 256)")
        words[t >> 5] |= 1 << (t & 31)
    return (C.c_uint32 * 8)(*words)


def window_count(T: int, window: int, stride: int) -> int:
    """Sliding windows of one sequence of T positions (motif_extractor.py:13-17)."""
    return (T - window) // stride + 1 if T >= window else 0


def window_keep(idx, window, stride, exclude_ids=()):
    """int32 (B, nwin): 1 where no token of window j of idx (B, T) is in exclude_ids
    (motif_extractor.py:71-77)."""
    L.require_device(idx, "window_keep")
    idx = idx.to(torch.int64).contiguous()
    B, T = idx.shape
    if window < 1 or stride < 1:
        raise ValueError("window and stride must be at least 1")
    keep = torch.empty(B, window_count(T, window, stride), dtype=torch.int32, device=idx.device)
    L.check(L.lib.cg_window_keep(idx.data_ptr(), B, T, int(window), int(stride), _id_mask(exclude_ids, "exclude ids"),
                                 keep.data_ptr(), L.stream_ptr(idx.device)), "cg_window_keep")
    return keep


def window_pool(hidden, window, stride, dst_row, out):
    """Mean of hidden (B, T, d; fp32 or bf16, read in place) over every sliding window, written to
    row dst_row[b, j] of out (fp32, rows >= d wide); a row index outside out is skipped
    (motif_extractor.py:80-83).  Returns out."""
    for t in (hidden, dst_row, out):
        L.require_device(t, "window_pool")
    B, T, d = hidden.shape
    if hidden.stride(2) != 1 or hidden.stride(0) != T * hidden.stride(1):
        hidden = hidden.contiguous()
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != d or (out.shape[0] > 1 and out.stride(1) != 1):
        raise ValueError("window_pool: out must be fp32 (rows, d) with unit column stride")
    nwin = window_count(T, window, stride)
    if dst_row.dtype != torch.int32 or dst_row.numel() != B * nwin or not dst_row.is_contiguous():
        raise ValueError("window_pool: dst_row must be a contiguous int32 (B, nwin)")
    L.check(L.lib.cg_window_pool(_dt(hidden), hidden.data_ptr(), hidden.stride(1), B, T, d, int(window), int(stride),
                                 dst_row.data_ptr(), out.data_ptr(), out.stride(0), out.shape[0],
                                 L.stream_ptr(hidden.device)), "cg_window_pool")
    return out


class KMeansStep(_Result):
    """Outputs of kmeans_step; an output that was not asked for is None."""
    __slots__ = ("labels", "dist2", "sums", "counts", "inertia")


def kmeans_step(x, centers, *, want_dist2=True, want_stats=True, want_inertia=True, workspace=None):
    """One E-step of Lloyd's algorithm with the M-step's statistics (cg_kmeans_step): labels int32
    (n), dist2 fp32 (n), sums fp64 (k, d), counts int64 (k), inertia fp64 scalar tensor.  x fp32
    (n, d) and centers fp32 (k, d) may have padded rows.  workspace: a uint8 buffer to reuse."""
    ld = []
    for name, t in (("x", x), ("centers", centers)):
        L.require_device(t, "kmeans_step")
        ld.append(_row_matrix(t, f"kmeans_step: {name}", loose=True))
    n, d = x.shape
    k = centers.shape[0]
    if centers.shape[1] != d:
        raise ValueError("kmeans_step: points and centres differ in width")
    dev = x.device
    p = L.KMeansDesc()
    p.x, p.ldx, p.n, p.d = x.data_ptr(), ld[0], n, d
    p.centers, p.ldc, p.k = centers.data_ptr(), ld[1], k
    r = KMeansStep(labels=torch.empty(n, dtype=torch.int32, device=dev))
    if want_dist2:
        r.dist2 = torch.empty(n, dtype=torch.float32, device=dev)
    if want_stats:
        r.sums = torch.zeros(k, d, dtype=torch.float64, device=dev)
        r.counts = torch.zeros(k, dtype=torch.int64, device=dev)
    if want_inertia:
        r.inertia = torch.zeros((), dtype=torch.float64, device=dev)
    p.labels, p.dist2, p.sums, p.counts, p.inertia = _p(r.labels), _p(r.dist2), _p(r.sums), _p(r.counts), _p(r.inertia)
    _set_ws(p, _pick_ws(workspace, dev, "u8", True, L.lib.cg_kmeans_workspace, n, d, k))
    L.check(L.lib.cg_kmeans_step(C.byref(p), L.stream_ptr(dev)), "cg_kmeans_step")
    return r


class TermCE:
    """State of term_ce_fwd: ``loss`` (0-d fp32) and ``sums`` (2,) = (sum w nll, sum w), and the
    operands and workspace term_ce_bwd reads again."""
    __slots__ = ("loss", "sums", "x", "W", "bias", "labels", "class_w", "ignore_index", "workspace")


def _term_ce_desc(st: TermCE):
    x, W = st.x, st.W
    p = L.TermCeDesc()
    p.x_dtype, p.x = _dt(x), x.data_ptr()
    p.ldx = _row_matrix(x, "term_ce: x", (torch.float32, torch.bfloat16), loose=True)
    p.rows, p.d, p.C = x.shape[0], x.shape[1], W.shape[0]
    p.W, p.ldw = W.data_ptr(), _row_matrix(W, "term_ce: W", loose=True)
    p.bias, p.labels, p.ignore_index, p.class_w = st.bias.data_ptr(), st.labels.data_ptr(), st.ignore_index, _p(st.class_w)
    _set_ws(p, st.workspace)
    return p


def term_ce_fwd(x, W, bias, labels, *, class_w=None, ignore_index=-100, workspace=None) -> TermCE:
    """Fused termination-head loss (cg_term_ce_fwd): the class-weighted cross-entropy of
    x W^T + bias against labels over the labelled rows, without materialising the logits.
    x (rows, d) fp32 or bf16, W fp32 (C, d), C <= 16, bias fp32 (C), labels int64 (rows), class_w
    fp32 (C) or None; x and W may have padded rows.  A label equal to ignore_index or outside
    [0, C) is ignored.  No labelled row: the loss is NaN.  Returns the state term_ce_bwd takes."""
    for t in (x, W, bias, labels) + (() if class_w is None else (class_w,)):
        L.require_device(t, "term_ce_fwd")
    if x.dim() != 2 or W.dim() != 2:
        raise ValueError("term_ce_fwd: x (rows, d) and W (C, d)")
    rows, d = x.shape
    nc = W.shape[0]
    if W.shape[1] != d or bias.numel() != nc or labels.numel() != rows or (class_w is not None and class_w.numel() != nc):
        raise ValueError("term_ce_fwd: x (rows, d), W (C, d), bias (C), labels (rows), class_w (C)")
    dev = x.device
    st = TermCE()
    st.x, st.W = x, W
    st.bias = bias.to(torch.float32).contiguous()
    st.labels = labels.reshape(-1).to(torch.int64).contiguous()  # device and count checked above
    st.class_w = None if class_w is None else class_w.to(torch.float32).contiguous()
    st.ignore_index = int(ignore_index)
    st.loss = torch.empty((), dtype=torch.float32, device=dev)
    st.sums = torch.empty(2, dtype=torch.float32, device=dev)
    st.workspace = _pick_ws(workspace, dev, "u8", True, L.lib.cg_term_ce_workspace, rows, d,
                            min(nc, L.TERM_CE_MAX_CLASSES))
    p = _term_ce_desc(st)
    p.loss, p.sums = st.loss.data_ptr(), st.sums.data_ptr()
    L.check(L.lib.cg_term_ce_fwd(C.byref(p), L.stream_ptr(dev)), "cg_term_ce_fwd")
    return st


def term_ce_bwd(st: TermCE, *, scale=1.0, scale_dev=None, dW=None, db=None, dx=None, want=("dW", "db", "dx")):
    """Backward of term_ce_fwd (cg_term_ce_bwd): g = scale * scale_dev * w_y (softmax - onehot) /
    sum w on the labelled rows; dW (C, d) = g^T x, db (C) = column sums of g, dx (rows, d) = g W,
    all fp32.  A tensor passed as dW / db / dx is ACCUMULATED into (and returned); an output named
    in ``want`` and not passed is allocated and overwritten (dx: zero on unlabelled rows).
    scale_dev: an optional one-element fp32 device tensor, read in the kernel.  Returns (dW, db, dx)
    with None for outputs neither passed nor wanted."""
    rows, d = st.x.shape
    nc = st.W.shape[0]
    dev = st.x.device
    p = _term_ce_desc(st)
    p.scale = float(scale)
    if scale_dev is not None:
        L.require_device(scale_dev, "term_ce_bwd")
        scale_dev = scale_dev.detach().reshape(1).to(torch.float32).contiguous()
        p.scale_dev = scale_dev.data_ptr()
    shapes = {"dW": (nc, d), "db": (nc,), "dx": (rows, d)}
    outs = {}
    for name, t in (("dW", dW), ("db", db), ("dx", dx)):
        acc = t is not None
        if t is None and name in want:
            t = torch.empty(shapes[name], dtype=torch.float32, device=dev)
        outs[name] = t
        if t is None:
            continue
        L.require_device(t, "term_ce_bwd")
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"term_ce_bwd: {name} must have shape {shapes[name]}")
        setattr(p, name, t.data_ptr())
        setattr(p, "acc_" + name, int(acc))
        if name == "db":
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("term_ce_bwd: db must be contiguous fp32")
        else:
            setattr(p, "ld" + name.lower(), _row_matrix(t, f"term_ce_bwd: {name}", loose=True))
    L.check(L.lib.cg_term_ce_bwd(C.byref(p), L.stream_ptr(dev)), "cg_term_ce_bwd")
    return outs["dW"], outs["db"], outs["dx"]


class NgramTables:
    """Device int64 count tables of the segment-aware n-gram baselines (cg_ngram_count) and, after
    ngram_totals, their row totals.  ``n_bad`` counts positions skipped for a token outside [0, V)."""
    __slots__ = ("V", "pad_id", "reset_ids", "uni", "bi", "tri", "n_bad", "uni_total", "bi_total", "tri_total")

    def __init__(self, V, device, pad_id=0, reset_ids=()):
        V = int(V)
        if V > L.NGRAM_MAX_V:
            raise ValueError(f"n-gram tables: V = {V} exceeds {L.NGRAM_MAX_V} (CG_EUNSUPPORTED)")
        if not torch.device(device).type == "cuda":
            raise RuntimeError("n-gram tables live on the MI355X; codonlm_amd has no CPU path")
        self.V, self.pad_id, self.reset_ids = V, int(pad_id), tuple(sorted(int(t) for t in reset_ids))
        self.uni = torch.zeros(V, dtype=torch.int64, device=device)
        self.bi = torch.zeros(V, V, dtype=torch.int64, device=device)
        self.tri = torch.zeros(V, V, V, dtype=torch.int64, device=device)
        self.n_bad = torch.zeros(1, dtype=torch.int64, device=device)
        self.uni_total = self.bi_total = self.tri_total = None


def _xy(x, y, what):
    L.require_device(x, what)
    L.require_device(y, what)
    if x.dim() != 2 or x.shape != y.shape:
        raise ValueError(f"{what}: x and y are [B][T]")
    return x.to(torch.int64).contiguous(), y.to(torch.int64).contiguous()


def ngram_count(tables: NgramTables, x, y):
    """cg_ngram_count: add the counted positions of x, y (device int64 [B][T]) to ``tables``
    (fit_baselines of the reference's eval_ppl_baselines.py).  The totals become stale."""
    x, y = _xy(x, y, "ngram_count")
    B, T = x.shape
    L.check(L.lib.cg_ngram_count(x.data_ptr(), y.data_ptr(), B, T, tables.V, tables.pad_id,
                                 _id_mask(tables.reset_ids, "reset ids"), tables.uni.data_ptr(), tables.bi.data_ptr(),
                                 tables.tri.data_ptr(), tables.n_bad.data_ptr(), L.stream_ptr(x.device)),
            "cg_ngram_count")
    tables.uni_total = tables.bi_total = tables.tri_total = None
    return tables


def ngram_totals(tables: NgramTables):
    """cg_ngram_totals: the row totals over the targets 1 .. V-1, once after fitting."""
    V, dev = tables.V, tables.uni.device
    tables.uni_total = torch.empty(1, dtype=torch.int64, device=dev)
    tables.bi_total = torch.empty(V, dtype=torch.int64, device=dev)
    tables.tri_total = torch.empty(V, V, dtype=torch.int64, device=dev)
    L.check(L.lib.cg_ngram_totals(tables.uni.data_ptr(), tables.bi.data_ptr(), tables.tri.data_ptr(), V,
                                  tables.uni_total.data_ptr(), tables.bi_total.data_ptr(),
                                  tables.tri_total.data_ptr(), L.stream_ptr(dev)), "cg_ngram_totals")
    return tables


class NgramNll(_Result):
    """Device tensors of one ngram_nll call; an output that was not asked for is None."""
    __slots__ = ("tok_tri", "row_sums", "row_count", "acc")


NGRAM_OUTPUTS = ("tok_tri", "row_sums", "row_count")


def ngram_nll(tables: NgramTables, x, y, alpha=0.01, *, acc=None, want=("row_sums", "row_count"), workspace=None):
    """cg_ngram_nll of x, y (device int64 [B][T]) under ``tables`` (evaluate_baselines / _trigram_nll of
    the reference): ``tok_tri`` fp32 [B][T], ``row_sums`` fp64 [B][4] (uniform, unigram, bigram,
    trigram), ``row_count`` int32 [B], and ``acc``: the fp64 [5] accumulator the launch added to."""
    x, y = _xy(x, y, "ngram_nll")
    _check_want("ngram_nll", want, NGRAM_OUTPUTS)
    if tables.uni_total is None:
        raise ValueError("ngram_nll: call ngram_totals after the last ngram_count")
    B, T = x.shape
    dev = x.device
    d = L.NgramNllDesc()
    d.x, d.y, d.B, d.T, d.V, d.pad_id = x.data_ptr(), y.data_ptr(), B, T, tables.V, tables.pad_id
    d.reset_mask = _id_mask(tables.reset_ids, "reset ids")
    d.alpha = float(alpha)
    for name in ("uni", "bi", "tri", "uni_total", "bi_total", "tri_total"):
        setattr(d, name, getattr(tables, name).data_ptr())
    res = NgramNll()
    _alloc_outputs(d, res, want, dev, (("tok_tri", (B, T), torch.float32), ("row_sums", (B, 4), torch.float64),
                                       ("row_count", B, torch.int32)))
    if acc is not None:  # the workspace holds the accumulator's partials: set only with one
        res.acc, d.acc = acc, _dev_tensor(acc, torch.float64, 5, "ngram_nll: acc")
        _set_ws(d, _pick_ws(workspace, dev, "f64", False, L.lib.cg_ngram_nll_workspace, B))
    L.check(L.lib.cg_ngram_nll(C.byref(d), L.stream_ptr(dev)), "cg_ngram_nll")
    return res


class DiagResult(_Result):
    """Device tensors of one diag_rows call; an output that was not asked for is None."""
    __slots__ = ("nll", "segpos", "conf", "row_nll", "row_count", "slices", "calib", "brier_acc")


DIAG_OUTPUTS = ("nll", "segpos", "conf", "row_nll", "row_count")


def diag_workspace(B, device):
    """A cg_diag_rows workspace for up to ``B`` rows (8-byte aligned)."""
    return _alloc_ws(L.lib.cg_diag_workspace(int(B)), device, "f64")


def diag_rows(logits, x, y, *, V=None, pad_id=0, sep_id=3, row_flag=None, tok_class=None, edges=None, slices=None,
              calib=None, brier_acc=None, want=(), workspace=None):
    """cg_diag_rows over the fp32 logits [B*T][ld] of a forward over x with the targets y (device int64
    [B][T]): the loss slices, calibration bins and Brier sums the reference's diagnose_context_learning.py
    and calibration_metrics.py take in Python loops.  ``slices`` fp64 [13][2], ``calib`` fp64
    [n_bins][3] (with ``edges`` fp32 [n_bins + 1]) and ``brier_acc`` fp64 [2] are device accumulators
    the launch adds to; ``want`` names per-token (nll, segpos, conf: [B][T]) and per-row (row_nll fp64,
    row_count int32: [B]) outputs."""
    L.require_device(logits, "diag_rows")
    x, y = _xy(x, y, "diag_rows")
    B, T = x.shape
    ldl = _row_matrix(logits, "diag_rows: logits", width=V)
    if logits.shape[0] != B * T:
        raise ValueError("diag_rows: logits has one row per position of x, [B*T][ld]")
    _check_want("diag_rows", want, DIAG_OUTPUTS)
    V = logits.shape[1] if V is None else int(V)
    dev = logits.device
    d = L.DiagDesc()
    d.logits, d.ldl = logits.data_ptr(), ldl
    d.x, d.y, d.B, d.T, d.V, d.pad_id, d.sep_id = x.data_ptr(), y.data_ptr(), B, T, V, int(pad_id), int(sep_id)
    if row_flag is not None:
        d.row_flag = _dev_tensor(row_flag, torch.uint8, B, "diag_rows: row_flag")
    if tok_class is not None:
        d.tok_class = _dev_tensor(tok_class, torch.uint8, V, "diag_rows: tok_class")
    res = DiagResult()
    if edges is not None:
        n_bins = edges.numel() - 1
        d.edges, d.n_bins = _dev_tensor(edges, torch.float32, n_bins + 1, "diag_rows: edges"), n_bins
        if calib is not None:
            d.calib = _dev_tensor(calib, torch.float64, 3 * n_bins, "diag_rows: calib")
    elif calib is not None:
        raise ValueError("diag_rows: calib needs edges")
    if slices is not None:
        d.slices = _dev_tensor(slices, torch.float64, 2 * len(L.DIAG_SLICES), "diag_rows: slices")
    if brier_acc is not None:
        d.brier_acc = _dev_tensor(brier_acc, torch.float64, 2, "diag_rows: brier_acc")
    res.slices, res.calib, res.brier_acc = slices, calib, brier_acc
    _alloc_outputs(d, res, want, dev, (
        ("nll", (B, T), torch.float32), ("segpos", (B, T), torch.int32), ("conf", (B, T), torch.float32),
        ("row_nll", B, torch.float64), ("row_count", B, torch.int32)))
    if slices is not None or calib is not None or brier_acc is not None:  # a workspace only with an accumulator
        _set_ws(d, _pick_ws(workspace, dev, "f64", False, L.lib.cg_diag_workspace, B))
    L.check(L.lib.cg_diag_rows(C.byref(d), L.stream_ptr(dev)), "cg_diag_rows")
    return res


class AttnStatsResult(_Result):
    """Device tensors of one attn_stats call; an output that was not asked for is None."""
    __slots__ = ("rows", "nvis", "received", "head_acc", "n_rows")


ATTN_STATS_OUTPUTS = ("rows", "nvis", "received")


def attn_stats_workspace(B, T, H, device):
    """A cg_attn_stats workspace for (B, T, H) (8-byte aligned)."""
    return _alloc_ws(L.lib.cg_attn_stats_workspace(int(B), int(T), int(H)), device, "f64")


def attn_stats_fill(d, res, B, T, H, dev, *, idx=None, pad_id=-1, tok_class=None, row_keep=None,
                    want=ATTN_STATS_OUTPUTS, head_acc=None, n_rows=None, workspace=None):
    """The fields of an AttnStatsDesc a caller chooses (token ids, classes, row filter, outputs,
    workspace), shared by attn_stats and Engine.attn_stats; returns the tensors to keep alive."""
    _check_want("attn_stats", want, ATTN_STATS_OUTPUTS)
    keep = []
    if idx is not None:
        idx = idx.to(device=dev, dtype=torch.int64).contiguous()
        d.idx = _dev_tensor(idx, torch.int64, B * T, "attn_stats: idx")
        keep.append(idx)
    d.pad_id = int(pad_id)
    if tok_class is not None:
        d.tok_class, d.V = _dev_tensor(tok_class, torch.uint8, tok_class.numel(), "attn_stats: tok_class"), tok_class.numel()
    if row_keep is not None:
        row_keep = row_keep.to(device=dev, dtype=torch.uint8).contiguous()
        d.row_keep = _dev_tensor(row_keep, torch.uint8, B * T, "attn_stats: row_keep")
        keep.append(row_keep)
    _alloc_outputs(d, res, want, dev, (("rows", (B, H, T, L.AS_NSTAT), torch.float32), ("nvis", (B, T), torch.int32),
                                       ("received", (B, H, T), torch.float32)))
    if head_acc is not None:
        d.head_acc = _dev_tensor(head_acc, torch.float64, H * L.AS_NSTAT, "attn_stats: head_acc")
    if n_rows is not None:
        d.n_rows = _dev_tensor(n_rows, torch.float64, 1, "attn_stats: n_rows")
    res.head_acc, res.n_rows = head_acc, n_rows
    ws = _pick_ws(workspace, dev, "f64", False, L.lib.cg_attn_stats_workspace, B, T, H)
    _set_ws(d, ws)
    keep.append(ws)
    return keep


def attn_stats(qkv, segstart, B, T, H, KV, hd, *, window=0, idx=None, pad_id=-1, tok_class=None, row_keep=None,
               want=ATTN_STATS_OUTPUTS, head_acc=None, n_rows=None, workspace=None):
    """cg_attn_stats over the qkv rows [B*T][(H + 2 KV) hd] of a forward (RoPE applied): the per-row
    statistics of the attention probabilities (``rows`` fp32 [B][H][T][14] in the order of
    L.AS_STATS), ``nvis`` int32 [B][T], ``received`` fp32 [B][H][T], and the device accumulators
    ``head_acc`` fp64 [H][14] and ``n_rows`` fp64 [1] the launch adds to.  No T x T tensor is
    written.  ``idx`` int64 [B][T] with ``pad_id`` drops PAD rows and, with ``tok_class`` uint8 [V],
    gives the key classes; ``row_keep`` uint8 [B][T] filters the query rows."""
    L.require_device(qkv, "attn_stats")
    # not _row_matrix: any dtype _dt takes, and "empty" is numel() == 0 with the stride (H + 2 KV) hd
    if qkv.dim() != 2 or qkv.shape[0] != B * T or (qkv.numel() and qkv.stride(1) != 1):
        raise ValueError("attn_stats: qkv is [B*T][(H + 2 KV) hd] with contiguous rows")
    dev = qkv.device
    d = L.AttnStatsDesc()
    d.dtype, d.qkv, d.ldqkv = _dt(qkv), qkv.data_ptr(), qkv.stride(0) if qkv.numel() else (H + 2 * KV) * hd
    d.segstart = _p(segstart)
    d.B, d.T, d.H, d.KV, d.hd, d.window = B, T, H, KV, hd, int(window or 0)
    res = AttnStatsResult()
    keep = attn_stats_fill(d, res, B, T, H, dev, idx=idx, pad_id=pad_id, tok_class=tok_class, row_keep=row_keep,
                           want=want, head_acc=head_acc, n_rows=n_rows, workspace=workspace)
    L.check(L.lib.cg_attn_stats(C.byref(d), L.stream_ptr(dev)), "cg_attn_stats")
    del keep
    return res


# ---------------------------------------------------------------------------- structural regression probes
SHAPE_TARGETS = L.SHAPE_TARGETS


def _rows_view(t, what):
    """(tensor kept alive, rows, width, row stride) of a (rows, w) or (B, T, w) tensor whose rows are
    evenly spaced with unit column stride (a column slice of a wider buffer included)."""
    if t.dim() == 3:
        B, T, w = t.shape
        if B > 1 and T > 0 and t.stride(0) != T * t.stride(1):
            t = t.contiguous()
        rows, ld = B * T, t.stride(1)
    elif t.dim() == 2:
        rows, w = t.shape
        ld = t.stride(0)
    else:
        raise ValueError(f"{what}: a (rows, w) or (B, T, w) tensor")
    if w > 1 and t.stride(-1) != 1:
        raise ValueError(f"{what}: unit column stride")
    return t, rows, w, max(int(ld), w)


def shape_targets(idx, codon_of, out=None):
    """(y fp32 (B*T, 14), valid int32 (B*T)): the per-codon DNAshape targets of idx int64 (B, T)
    (cg_shape_targets).  codon_of: one int per id, 6 bits = three 2-bit nucleotides (A, C, G, T =
    0..3, first in the high bits), negative = not a codon.  Rows of non-codon positions are left as
    they are (zeros in a fresh y).  out: a (B*T, >= 14) fp32 buffer to write into."""
    L.require_device(idx, "shape_targets")
    if idx.dim() != 2:
        raise ValueError("shape_targets: idx is (B, T)")
    idx = idx.to(torch.int64).contiguous()
    B, T = idx.shape
    tab = [int(v) for v in codon_of]
    if len(tab) > 256:
        raise ValueError("shape_targets: at most 256 ids")
    y = torch.zeros(B * T, SHAPE_TARGETS, dtype=torch.float32, device=idx.device) if out is None else out
    # not _row_matrix: numel() decides "empty", and the stride is raised to the width for every row count
    if y.dtype != torch.float32 or y.dim() != 2 or y.shape[0] != B * T or (y.numel() and y.stride(1) != 1):
        raise ValueError("shape_targets: out must be fp32 (B*T, >= 14) with unit column stride")
    ldy = max(int(y.stride(0)), y.shape[1]) if y.shape[1] else 0
    valid = torch.empty(B * T, dtype=torch.int32, device=idx.device)
    L.check(L.lib.cg_shape_targets(idx.data_ptr(), B, T, (C.c_int32 * max(len(tab), 1))(*tab), len(tab),
                                   y.data_ptr(), ldy, valid.data_ptr(), L.stream_ptr(idx.device)),
            "cg_shape_targets")
    return y, valid


def gram_workspace(rows, d, m, G, device):
    """A cg_gram_accum workspace for these sizes (a uint8 tensor)."""
    return _alloc_ws(L.lib.cg_gram_workspace(int(rows), int(d), int(m), int(G)), device, "u8_256")


def gram_accum(h, y, grp, G, gram=None, *, m=None, accumulate=False, workspace=None):
    """gram fp64 (G, P, P), P = d + m + 1: per group g the sum over the rows r with grp[r] == g of
    z z^T, z = (h[r], y[r][:m], 1), accumulated in fp64 on the f64 MFMA (cg_gram_accum).  h: (rows, d)
    or (B, T, d), fp32 or bf16, read in place; y: fp32 (rows, >= m) or None (m = 0); grp int32
    (rows), rows with a value outside [0, G) are skipped and never read.  gram: the matrix to
    overwrite (accumulate=False) or add to (accumulate=True); a (G, P, >= P) view of a wider
    buffer is allowed.  workspace: a uint8 buffer to reuse (gram_workspace)."""
    L.require_device(h, "gram_accum")
    L.require_device(grp, "gram_accum")
    h, rows, d, ldh = _rows_view(h, "gram_accum: h")
    dev = h.device
    if y is None:
        if m not in (None, 0):
            raise ValueError("gram_accum: m columns asked of no y")
        m, ldy, yk = 0, 0, None
    else:
        L.require_device(y, "gram_accum")
        if y.dtype != torch.float32:
            raise ValueError("gram_accum: y must be fp32")
        yk, yrows, wy, ldy = _rows_view(y, "gram_accum: y")
        m = wy if m is None else int(m)
        if yrows != rows or m > wy or m < 0:
            raise ValueError("gram_accum: y must have h's rows and at least m columns")
    if grp.dtype != torch.int32 or grp.numel() != rows or not grp.is_contiguous():
        raise ValueError("gram_accum: grp must be a contiguous int32 (rows)")
    G = int(G)
    if G < 1:
        raise ValueError("gram_accum: at least one group")
    P = d + m + 1
    if gram is None:
        if accumulate:
            raise ValueError("gram_accum: accumulate needs a gram to add to")
        gram = torch.empty(G, P, P, dtype=torch.float64, device=dev)
    L.require_device(gram, "gram_accum")
    if (gram.dtype != torch.float64 or gram.dim() != 3 or tuple(gram.shape) != (G, P, P) or gram.stride(2) != 1
            or (G > 1 and gram.stride(0) != P * gram.stride(1))):
        raise ValueError("gram_accum: gram must be fp64 (G, P, P) with evenly spaced rows")
    ws = _pick_ws(workspace, dev, "u8_256", True, L.lib.cg_gram_workspace, rows, d, m, G)
    L.check(L.lib.cg_gram_accum(_dt(h), h.data_ptr(), ldh, d, _p(yk), ldy, m, grp.data_ptr(), rows, G,
                                1 if accumulate else 0, gram.data_ptr(), max(int(gram.stride(1)), P), ws.data_ptr(),
                                _nbytes(ws), L.stream_ptr(dev)), "cg_gram_accum")
    return gram


def _seq_set(sym, offsets, what):
    """(device uint8 flat symbols, device int64 offsets, host int64 offsets) of a sequence set; offsets may be
    a host array or a device tensor (read back once)."""
    L.require_device(sym, what)
    if sym.dtype != torch.uint8 or sym.dim() != 1 or not sym.is_contiguous():
        raise ValueError(f"{what}: symbols are a flat contiguous uint8 tensor")
    if sym.data_ptr() % 4:
        raise ValueError(f"{what}: the symbol buffer must be 4-byte aligned")
    host = (offsets.cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)).astype(np.int64)
    if host.ndim != 1 or host.size < 1 or (np.diff(host) < 0).any() or host[0] < 0 or host[-1] > sym.numel():
        raise ValueError(f"{what}: offsets are non-decreasing, start at or after 0 and end within the symbols")
    if sym.numel() > L.NGRAM_INDEX_MAX_SYM:
        raise ValueError(f"{what}: more than 2^32 - 2 symbols (CG_EUNSUPPORTED)")
    dev_off = offsets if isinstance(offsets, torch.Tensor) and offsets.is_cuda and offsets.dtype == torch.int64 \
        else torch.from_numpy(host).to(sym.device)
    return sym, dev_off.contiguous(), host


def ngram_window_count(offsets, n: int, lo: int = 0, hi=None) -> int:
    """The number of windows of n symbols of the sequences [lo, hi) of host ``offsets``."""
    lens = np.diff(np.asarray(offsets, dtype=np.int64))[lo:hi]
    return int(np.maximum(lens - int(n) + 1, 0).sum())


class NgramIndex:
    """An exact window-membership index over the sequence set (``sym`` device uint8, ``offsets``
    int64 [n_seq + 1]) for windows of ``n`` symbols: the open-addressing ``table`` of
    cg_ngram_index_build (uint32 [capacity], filled with empty slots here), ``n_unique`` (device int64 [1],
    the distinct windows inserted so far) and ``n_dropped`` (stays 0).  The default capacity is the
    smallest power of two >= 2 x the windows of the whole set; ``capacity=`` overrides it (a power of two
    above the window count)."""
    __slots__ = ("sym", "offsets", "host_offsets", "n", "table", "capacity", "n_unique", "n_dropped")

    def __init__(self, sym, offsets, n: int, capacity=None):
        n = int(n)
        if not 1 <= n <= L.NGRAM_INDEX_MAX_N:
            raise ValueError(f"ngram index: window of {n} symbols outside 1..{L.NGRAM_INDEX_MAX_N}")
        self.sym, self.offsets, self.host_offsets = _seq_set(sym, offsets, "ngram index")
        self.n = n
        windows = ngram_window_count(self.host_offsets, n)
        if capacity is None:
            capacity = 2
            while capacity < 2 * windows:
                capacity *= 2
        capacity = int(capacity)
        if capacity < 2 or capacity & (capacity - 1) or capacity <= windows or capacity > 2 ** 32:
            raise ValueError(f"ngram index: capacity {capacity} must be a power of two in 2..2^32 above the "
                             f"{windows} windows of the set")
        dev = sym.device
        self.capacity = capacity
        # 0xFFFFFFFF = the empty slot
        self.table = torch.full((capacity,), -1, dtype=torch.int32, device=dev)
        self.n_unique = torch.zeros(1, dtype=torch.int64, device=dev)
        self.n_dropped = torch.zeros(1, dtype=torch.int64, device=dev)

    @property
    def n_seq(self) -> int:
        return int(self.host_offsets.size - 1)


def ngram_index_build(index: NgramIndex, seq_lo: int = 0, seq_hi=None) -> NgramIndex:
    """cg_ngram_index_build: insert every window of the sequences [seq_lo, seq_hi) (default: all) of the
    index's own set.  Launches over disjoint ranges add up to the build of their union; inserting a
    range twice leaves the set and ``n_unique`` unchanged."""
    seq_hi = index.n_seq if seq_hi is None else int(seq_hi)
    seq_lo = int(seq_lo)
    if not 0 <= seq_lo <= seq_hi <= index.n_seq:
        raise ValueError(f"ngram_index_build: sequences [{seq_lo}, {seq_hi}) outside 0..{index.n_seq}")
    d = L.NgramIndexDesc()
    d.sym, d.n_sym = index.sym.data_ptr(), index.sym.numel()
    d.offsets, d.n_seq, d.seq_lo, d.seq_hi = index.offsets.data_ptr(), index.n_seq, seq_lo, seq_hi
    d.n, d.table, d.capacity = index.n, index.table.data_ptr(), index.capacity
    d.n_unique, d.n_dropped = index.n_unique.data_ptr(), index.n_dropped.data_ptr()
    L.check(L.lib.cg_ngram_index_build(C.byref(d), L.stream_ptr(index.sym.device)), "cg_ngram_index_build")
    return index


class NgramCoverage(_Result):
    """Device tensors of one ngram_coverage call; an output that was not asked for is None."""
    __slots__ = ("hit", "n_hit", "covered")


COVERAGE_OUTPUTS = ("hit", "n_hit", "covered")


def ngram_coverage(index: NgramIndex, qsym, qoffsets, want=("n_hit", "covered")) -> NgramCoverage:
    """cg_ngram_coverage of the query set (``qsym`` device uint8, ``qoffsets`` int64 [n_q + 1]) against a
    built index: ``hit`` uint8 like qsym (1 at the starts of windows the index holds), ``n_hit`` int32
    [n_q], ``covered`` int32 [n_q] (positions inside at least one hit window).  A query longer than
    16384 symbols raises ValueError (CG_EUNSUPPORTED)."""
    _check_want("ngram_coverage", want, COVERAGE_OUTPUTS)
    qsym, qoff, host = _seq_set(qsym, qoffsets, "ngram_coverage")
    n_q = int(host.size - 1)
    dev = qsym.device
    d = L.NgramCoverageDesc()
    d.sym, d.n_sym, d.n = index.sym.data_ptr(), index.sym.numel(), index.n
    d.table, d.capacity = index.table.data_ptr(), index.capacity
    d.qsym, d.n_qsym, d.qoffsets, d.n_q = qsym.data_ptr(), qsym.numel(), qoff.data_ptr(), n_q
    d.max_qlen = int(np.diff(host).max()) if n_q else 0
    res = NgramCoverage()
    _alloc_outputs(d, res, want, dev, (("hit", qsym.numel(), torch.uint8), ("n_hit", n_q, torch.int32),
                                       ("covered", n_q, torch.int32)), zero=("hit",))
    L.check(L.lib.cg_ngram_coverage(C.byref(d), L.stream_ptr(dev)), "cg_ngram_coverage")
    return res
