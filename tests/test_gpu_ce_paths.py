"""cg_cross_entropy against fp64 F.cross_entropy (ignore_index, label_smoothing, weight) on the
paths the 517-row test does not reach: the 16-row and 4-row loops of the denominator kernel and
the grid-strided main kernel (>= 16384 rows), the vocabulary edges of the two-values-per-lane
layout (V = 1, 64, 65, 128), ignore_index = -100, grad_scale, and the values of the bf16 and
split-bf16 (hi | lo) gradient layouts.

Every test needs the MI355X (marker ``gpu``) and calls the C ABI through codonlm_amd.ops.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _ops():
    from codonlm_amd import ops
    return ops


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(rows, V, ldl, eps, weighted, ignore_index, seed=11):
    """(logits CPU [rows][ldl] fp32, targets, weight or None, fp64 loss, fp64 grads [rows][V]):
    computed once and shared; callers must not modify it."""
    g = torch.Generator().manual_seed(seed + rows + V)
    full = torch.randn(rows, ldl, generator=g) * 5
    t = torch.randint(0, V, (rows,), generator=g)
    drop = torch.rand(rows, generator=g) < 0.1
    drop[0] = True
    drop[rows - 1] = False
    t[drop] = ignore_index
    if ignore_index >= 0:
        drop = t == ignore_index
    w = torch.rand(V, generator=g) + 0.5 if weighted else None
    zr = full[:, :V].double().clone().requires_grad_(True)
    ref = F.cross_entropy(zr, t, ignore_index=ignore_index, label_smoothing=eps,
                          weight=None if w is None else w.double())
    ref.backward()
    return full, t, w, ref.item(), zr.grad.detach(), drop


def _run(case, V, ignore_index, eps, **kw):
    full, t, w = case[:3]
    z = full.to(DEV)[:, :V]
    loss, dl = _ops().cross_entropy(z, t.to(DEV), eps=eps, weight=None if w is None else w.to(DEV),
                                    ignore_index=ignore_index, **kw)
    torch.cuda.synchronize()
    return loss.item(), dl.cpu()


ROWS_BIG = 16384 + 4096 + 517


@pytest.mark.parametrize("layout", ["f32", "bf16", "bf16x2"])
def test_ce_large_row_count(layout):
    """20997 rows: ce_denom_kernel runs one 16-row round, one 4-row round and its tail, and
    ce_main_kernel's 4096 workgroups take a second row each.  V = 68 inside a row stride of 80,
    class weights, label smoothing 0.1, about 10 % of the targets ignored.  Loss within 1e-5
    relative.  Gradients: fp32 within 1e-6 absolute (the 517-row test's tolerance) and, since
    every gradient here is below 1e-4, also within 1e-5 w_max / sum_valid(w_y): the per-row
    gradient before the division is a difference of probabilities and class weights of size
    <= w_max, computed in fp32 from __expf (below 1e-6 absolute on a probability) -- a bound that
    scales with the denominator.  bf16: 2^-8 |ref| + 1e-6; split bf16: hi + lo within
    2^-17 |ref| + 1e-6."""
    V, eps = 68, 0.1
    case = _case(ROWS_BIG, V, 80, eps, True, 0)
    full, t, w, ref_loss, ref_g, ignored = case
    kw = {"f32": dict(pad_to=80), "bf16": dict(pad_to=80, grad_dtype=torch.bfloat16),
          "bf16x2": dict(pad_to=160, split=True)}[layout]
    loss, dl = _run(case, V, 0, eps, **kw)
    rel = abs(loss - ref_loss) / abs(ref_loss)
    assert 0.05 < ignored.float().mean().item() < 0.15
    denom = w[t[~ignored]].double().sum().item()
    if layout == "f32":
        d = (dl[:, :V].double() - ref_g).abs()
        r_abs = (d / 1e-6).max().item()
        r_den = (d / (1e-5 * w.max().item() / denom)).max().item()
        print(f"ce large f32: loss rel/1e-5 {rel / 1e-5:.3f}, grad/1e-6 {r_abs:.4f}, grad/denominator bound {r_den:.3f}")
        assert r_abs <= 1.0 and r_den <= 1.0, (r_abs, r_den)
        assert torch.all(dl[:, V:] == 0)
        assert torch.all(dl[ignored] == 0)
    elif layout == "bf16":
        r = ((dl[:, :V].double() - ref_g).abs() / (2.0 ** -8 * ref_g.abs() + 1e-6)).max().item()
        print(f"ce large bf16: grad err/bound {r:.4f}")
        assert r <= 1.0, r
        assert torch.all(dl[:, V:] == 0)
    else:
        val = dl[:, :V].double() + dl[:, 80:80 + V].double()
        r = ((val - ref_g).abs() / (2.0 ** -17 * ref_g.abs() + 1e-6)).max().item()
        print(f"ce large bf16x2: grad err/bound {r:.4f}")
        assert r <= 1.0, r
        assert torch.all(dl[:, V:80] == 0) and torch.all(dl[:, 80 + V:] == 0)
    assert rel <= 1e-5, rel


@pytest.mark.parametrize("V", [1, 64, 65, 128])
def test_ce_vocab_edges(V):
    """V = 1 (one lane, loss 0), 64 (the first value of every lane only), 65 (one lane's second
    value) and 128 (the largest supported), 300 rows, class weights, smoothing 0.1 and
    ignore_index = -100 (the auxiliary objectives' value, so that class 0 is a real class)."""
    eps = 0.1
    case = _case(300, V, V + 3, eps, True, -100)
    _, t, _, ref_loss, ref_g, ignored = case
    loss, dl = _run(case, V, -100, eps, pad_to=V + 5)
    assert ignored.any() and (t == 0).any()
    rel = abs(loss - ref_loss) / max(1.0, abs(ref_loss))
    r = ((dl[:, :V].double() - ref_g).abs() / 1e-6).max().item()
    print(f"ce V={V}: loss err/1e-5 {rel / 1e-5:.3f}, grad err/1e-6 {r:.4f}")
    assert rel <= 1e-5, rel
    assert r <= 1.0, r
    assert torch.all(dl[:, V:] == 0) and torch.all(dl[ignored] == 0)


def test_ce_vocab_too_large():
    z = torch.zeros(8, 129, device=DEV)
    t = torch.ones(8, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError):
        _ops().cross_entropy(z, t)


def test_ce_grad_scale():
    """grad_scale multiplies the gradient (bound 1e-6 grad_scale) and leaves the loss bit for bit."""
    V, eps, gs = 68, 0.05, 0.25
    case = _case(517, V, 68, eps, True, 0)
    ref_g = case[4]
    loss1, dl1 = _run(case, V, 0, eps)
    loss, dl = _run(case, V, 0, eps, grad_scale=gs)
    assert loss == loss1
    r = ((dl.double() - gs * ref_g).abs() / (1e-6 * gs)).max().item()
    r1 = ((dl1.double() - ref_g).abs() / 1e-6).max().item()
    print(f"ce grad_scale: err/bound {r:.4f} (scale 1: {r1:.4f})")
    assert r <= 1.0 and r1 <= 1.0, (r, r1)
    assert dl.abs().max().item() < 0.5 * dl1.abs().max().item()


def test_ce_bf16_and_split_layouts():
    """CG_BF16 gradients within 2^-8 |ref| + 1e-6 (bf16 rounding leaves <= 2^-9 relative).
    CG_BF16X2: the hi half (columns [0, ldd/2)) is the CG_BF16 output bit for bit, hi + lo (lo at
    column ldd/2 + c) matches the fp64 gradient to 2^-17 |ref| + 1e-6 (two roundings of 2^-9),
    and the pad columns [V, ldd/2) of both halves are exactly zero.  ignore_index = -100 rows
    are zero in every layout."""
    V, eps, ldd = 68, 0.1, 160
    case = _case(517, V, 72, eps, True, -100)
    ref_g, ignored = case[4], case[5]
    _, db = _run(case, V, -100, eps, pad_to=ldd // 2, grad_dtype=torch.bfloat16)
    _, dx = _run(case, V, -100, eps, pad_to=ldd, split=True)
    assert dx.dtype == torch.bfloat16 and tuple(dx.shape) == (517, ldd)
    rb = ((db[:, :V].double() - ref_g).abs() / (2.0 ** -8 * ref_g.abs() + 1e-6)).max().item()
    hi, lo = dx[:, :ldd // 2], dx[:, ldd // 2:]
    rx = ((hi[:, :V].double() + lo[:, :V].double() - ref_g).abs() / (2.0 ** -17 * ref_g.abs() + 1e-6)).max().item()
    print(f"ce bf16 err/bound {rb:.4f}, bf16x2 err/bound {rx:.4f}")
    assert rb <= 1.0, rb
    assert rx <= 1.0, rx
    assert torch.equal(_bits(hi), _bits(db))
    assert torch.all(hi[:, V:] == 0) and torch.all(lo[:, V:] == 0)
    assert torch.all(dx[ignored] == 0) and torch.all(db[ignored] == 0)
    # the low halves carry information: some are non-zero
    assert (lo[:, :V] != 0).any()


@pytest.mark.parametrize("ldd", [161, 134])
def test_ce_split_layout_errors(ldd):
    """An odd row stride, or halves narrower than V, are refused."""
    z = torch.zeros(8, 68, device=DEV)
    t = torch.ones(8, dtype=torch.long, device=DEV)
    with pytest.raises(ValueError):
        _ops().cross_entropy(z, t, pad_to=ldd, split=True)
